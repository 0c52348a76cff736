"""Static instruction mix of the Newton trip loop of the lane-group planar step kernel (K3', plg::Solve) MINUS its
nested slot loops (the do-while loops of RowsPass and LineEval), i.e. the fixed part of a trip, per instruction category
and per segment between the slot loops.
usage: python tools/isa_trip.py file.s [kernel-name-substring ...]   (file.s: hipcc -S --cuda-device-only, the
Makefile's flags; default kernels: the four lane-group instantiations of the benchmark models)

The trip loop is found as the smallest loop (backward-branch range) that holds two or more innermost loops of at least
60 instructions, one of them with an LDS store (RowsPass<true> writes the line-search cache); the innermost loops in it
are the slot loops.  Segments: `head` = top of the trip up to the RowsPass slot loop (accumulator zeroing, slot set),
`mid` = between the two slot loops (group sums, stop tests, factor / solve / products with M, line-search set-up),
`tail` = after the LineEval slot loop (line-search step, bracketing, the qacc / Ma updates, loop control)."""
import collections
import re
import sys

KERNELS = {"HalfCheetah <2,0,1>": "ILi2ELi0ELi1E", "HalfCheetah <4,0,1>": "ILi4ELi0ELi1E",
           "Walker2d <2,1,1>": "ILi2ELi1ELi1E", "Hopper <1,3,1>": "ILi1ELi3ELi1E"}
MIN_SLOT_LOOP = 60


def cat(x):
    if re.match(r"v_(fma|mul|add|fmac|max|min)_f64|v_(rcp|rsq|sqrt|div_scale|div_fmas|div_fixup|trig|fract|floor|ldexp"
                r"|frexp)\w*f64", x):
        return "fp64 arith"
    if x.startswith("v_cmp") and "f64" in x:
        return "fp64 compare"
    if x.startswith("v_cndmask"):
        return "select (cndmask)"
    if "dpp" in x:
        return "DPP move"
    if x.startswith("v_accvgpr"):
        return "AGPR <-> VGPR move"
    if x.startswith("v_mov") or x.startswith("v_pk_mov"):
        return "VGPR move"
    if x.startswith("ds_"):
        return "LDS"
    if x.startswith(("global_", "flat_", "scratch_", "buffer_")):
        return "global memory"
    if x.startswith("s_waitcnt"):
        return "s_waitcnt"
    if x.startswith("s_nop"):
        return "s_nop"
    if x.startswith(("s_cbranch", "s_branch")):
        return "branch"
    if x.startswith("s_"):
        return "other scalar"
    if x.startswith("v_cmp"):
        return "integer compare"
    if x.startswith("v_"):
        return "integer / bit VALU"
    return "other"


def kernels(txt):
    for m in re.finditer(r"\n(_Z\S+):[^\n]*\n(.*?)\n\.Lfunc_end", txt, re.S):
        yield m.group(1), m.group(2)


def parse(body):
    seq, labels = [], {}
    for l in body.split("\n"):
        if re.match(r"\.LBB\d+_\d+:", l):
            labels[l.split(":")[0]] = len(seq)
        elif l.startswith("\t") and not l.strip().startswith((".", ";")):
            seq.append(l.strip())
    loops = set()
    for i, l in enumerate(seq):
        mm = re.match(r"s_c?branch\w*\s+(\.LBB\d+_\d+)", l)
        if mm and mm.group(1) in labels and labels[mm.group(1)] <= i:
            loops.add((labels[mm.group(1)], i))
    return seq, sorted(loops)


def merge(ranges):  # union of overlapping [a, b] ranges (a loop with several latches)
    out = []
    for a, b in sorted(ranges):
        if out and a <= out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], b))
        else:
            out.append((a, b))
    return out


def inside(r, o):
    return o[0] <= r[0] and r[1] <= o[1] and r != o


def trip_loop(seq, loops):
    heads = {}  # one range per loop header (a loop with several latches)
    for l0, l1 in loops:
        heads[l0] = max(heads.get(l0, l1), l1)
    big = [l for l in heads.items() if l[1] - l[0] + 1 >= MIN_SLOT_LOOP]
    innermost = merge([l for l in big if not any(inside(o, l) for o in big)])
    best = None
    for l in big:
        slots = [r for r in innermost if inside(r, l)]
        if len(slots) >= 2 and any(x.startswith("ds_write") for r in slots for x in seq[r[0]:r[1] + 1]):
            if best is None or l[1] - l[0] < best[0][1] - best[0][0]:
                best = (l, slots)
    return best


def mix(xs):
    c = collections.Counter(cat(x.split()[0]) for x in xs)
    return sum(c.values()), c


def fmt(tot, c):
    return f"{tot:4d}: " + ", ".join(f"{k} {v}" for k, v in c.most_common())


def report(label, seq, loops):
    (a, b), slots = trip_loop(seq, loops)
    print(f"## {label}")
    tot, _ = mix(seq[a:b + 1])
    print(f"trip loop [{a}, {b}] {tot} instructions; slot loops " +
          ", ".join(f"[{s0}, {s1}] {s1 - s0 + 1}" for s0, s1 in slots))
    fixed, segs, cur = [], [], a
    names = ["head", "mid", "tail"] + [f"seg{i}" for i in range(3, 10)]
    for s0, s1 in slots + [(b + 1, b + 1)]:
        segs.append(seq[cur:s0])
        fixed += seq[cur:s0]
        cur = s1 + 1
    ft, fc = mix(fixed)
    print(f"fixed part {fmt(ft, fc)}")
    for n, s in zip(names, segs):
        print(f"  {n:4s} {fmt(*mix(s))}")
    # loops between the trip and its slot loops: the line-search loop (parent: its body runs once per trip; with the
    # one-evaluation search peeled, the exact-search fallback, which the benchmark never enters)
    heads = {}
    for l0, l1 in loops:
        if a < l0 and l1 < b:
            heads[l0] = max(heads.get(l0, l1), l1)
    for r0, r1 in merge([l for l in heads.items() if any(inside(sl, l) for sl in slots)]):
        n = r1 - r0 + 1 - sum(s1 - s0 + 1 for s0, s1 in slots if r0 <= s0 and s1 <= r1)
        print(f"  of the fixed part, in the line-search loop [{r0}, {r1}] (minus its slot loop): {n}")


def main():
    txt = open(sys.argv[1]).read()
    want = {k: k for k in sys.argv[2:]} if len(sys.argv) > 2 else KERNELS
    for label, sub in want.items():
        for name, body in kernels(txt):
            if sub in name:
                report(label, *parse(body))


if __name__ == "__main__":
    main()
