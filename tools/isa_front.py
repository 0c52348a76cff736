"""Static instruction mix of the forward pass of the lane-group planar step kernel (K3', mj_planar_lg.hip.h), per source
segment: the loop that runs one forward pass (the `frame_skip` loop of the Euler models, the stage loop of the RK4
ones), split by the source line each instruction comes from, and the end of the chunk behind it.
usage: python tools/isa_front.py [--src DIR] file.s [kernel-name-substring ...]
  (--src: the directory of the mj_planar_lg.hip.h / mujoco_planar_lg.hip the file was built from; default: the tree's)
  file.s: hipcc -S --cuda-device-only -gline-tables-only with the Makefile's flags for mujoco_planar_lg.hip (the line
  table only adds .loc directives: the instructions are those of the product build, see --check)
  python tools/isa_front.py --check plain.s lines.s: the two builds have the same instructions

Every instruction is booked to the segment of the last `.loc` of mj_planar_lg.hip.h / mujoco_planar_lg.hip in front
of it whose line lies in one of the ranges below; lines of the shared helpers (the lane vocabulary, In4 / V3 algebra,
SinCos, the DevCx accessors, ...) keep the segment they are called from.  The trip loop (tools/isa_trip.py) is booked
to `solve` whole."""
import collections
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_trip import KERNELS, cat, kernels, merge, inside, trip_loop  # noqa: E402

HDR, TU = "mj_planar_lg.hip.h", "mujoco_planar_lg.hip"


def segments(src):
    """[(file, first line, last line, segment)] from the source itself: function boundaries by their signatures."""
    def find(path, pat, start=0):
        lines = open(path).read().split("\n")
        for i in range(start, len(lines)):
            if re.search(pat, lines[i]):
                return i + 1
        raise SystemExit(f"{path}: no line matches {pat!r}")
    h, t = os.path.join(src, HDR), os.path.join(src, TU)
    kin = find(h, r"EPA_HD void Kinematics\(")
    smooth = find(h, r"EPA_HD void SmoothForces\(")
    cols = find(h, r"EPA_HD void ForChainCols\(")
    pair_cols = find(h, r"EPA_HD void ForPairCols\(")
    solve_end = find(h, r"^// mj_forward:")
    fwd = find(h, r"EPA_HD V Forward\(")
    refresh = find(h, r"cx\.Refresh\(\);", fwd)
    warm_in = find(h, r"qacc\[decltype\(ic\)::value\] = warm\[", fwd)
    solve_call = find(h, r"Solve<KL>\(", fwd)
    warm_out = find(h, r"warm\[decltype\(ic\)::value\] = qacc\[", fwd)
    euler = find(h, r"EPA_HD V StepEuler\(")
    rk4 = find(h, r"EPA_HD V StepRK4\(")
    rk4_fwd = find(h, r"it \+= Forward<KL>", rk4)
    step_loop = find(t, r"for \(int s = 0; s < task\.frame_skip; \+\+s\)")
    step_end = find(t, r"const double x_after = ", step_loop)
    reset = find(t, r"^  if \(reset\) \{")
    reset_end = find(t, r"^  \} else \{", reset)
    return [
        (HDR, kin - 2, smooth - 2, "Kinematics"),
        (HDR, smooth - 1, cols - 3, "SmoothForces"),
        (HDR, cols - 2, pair_cols - 3, "MakeConstraint"),
        (HDR, pair_cols - 2, solve_end - 1, "solve"),
        (HDR, fwd, refresh, "Forward top"),
        (HDR, refresh + 1, warm_in - 1, "Forward top"),
        (HDR, warm_in, warm_in, "warm-start copies"),
        (HDR, solve_call, solve_call, "solve"),
        (HDR, warm_out, warm_out, "warm-start copies"),
        (HDR, euler, rk4 - 2, "integration"),
        (HDR, rk4, rk4_fwd - 1, "integration"),
        (HDR, rk4_fwd + 1, rk4_fwd + 30, "integration"),
        (TU, reset, reset_end, "reset branch"),
        (TU, step_loop, step_end - 1, "loop glue"),
        (TU, step_end, step_end + 70, "chunk end"),
    ]


def parse(body, files, segs):
    seq, src, labels = [], [], {}
    cur = "other"
    for l in body.split("\n"):
        s = l.strip()
        m = re.match(r"\.loc\s+(\d+)\s+(\d+)", s)
        if m:
            f, ln = files.get(int(m.group(1))), int(m.group(2))
            for sf, a, b, name in segs:
                if f == sf and a <= ln <= b:
                    cur = name
                    break
            continue
        if re.match(r"\.LBB\d+_\d+:", l):
            labels[l.split(":")[0]] = len(seq)
        elif l.startswith("\t") and not s.startswith((".", ";")):
            seq.append(s)
            src.append(cur)
    loops = set()
    for i, l in enumerate(seq):
        mm = re.match(r"s_c?branch\w*\s+(\.LBB\d+_\d+)", l)
        if mm and mm.group(1) in labels and labels[mm.group(1)] <= i:
            loops.add((labels[mm.group(1)], i))
    return seq, src, sorted(loops)


def fmt(xs):
    c = collections.Counter(cat(x.split()[0]) for x in xs)
    return f"{sum(c.values()):5d}: " + ", ".join(f"{k} {v}" for k, v in c.most_common())


ORDER = ["Forward top", "Kinematics", "SmoothForces", "MakeConstraint", "warm-start copies", "solve", "integration",
         "loop glue", "chunk end", "other"]


def report(label, seq, src, loops):
    (ta, tb), _ = trip_loop(seq, loops)
    heads = {}
    for l0, l1 in loops:
        heads[l0] = max(heads.get(l0, l1), l1)
    ranges = merge(list(heads.items()))
    # the forward-pass loop: the smallest loop around the trip loop that holds Kinematics code in front of the trip loop
    # and integration code behind it (the out-of-line blocks below branch back too, but end in front of the integration)
    fl = [r for r in heads.items() if r[0] < ta and tb < r[1] and "Kinematics" in src[r[0]:ta]
          and "integration" in src[tb + 1:r[1] + 1]]
    if not fl:  # block placement put part of the integration in front of the trip loop (or Kinematics behind it)
        fl = [r for r in heads.items() if r[0] < ta and tb < r[1] and "Kinematics" in src[r[0]:r[1] + 1]
              and "integration" in src[r[0]:r[1] + 1]]
    fa, fb = min(fl, key=lambda r: r[1] - r[0])
    print(f"## {label}")
    print(f"forward-pass loop [{fa}, {fb}] {fb - fa + 1} instructions; trip loop [{ta}, {tb}] {tb - ta + 1}")
    by = collections.defaultdict(list)
    for i in range(fa, fb + 1):
        by["solve" if ta <= i <= tb else src[i]].append(seq[i])
    outside = sum(len(v) for k, v in by.items() if k != "solve")
    print(f"  outside the trip loop {outside}")
    for k in ORDER:
        if by.get(k):
            print(f"  {k:18s} {fmt(by[k])}")
    # branches that jump backwards into the forward pass from behind the trip loop without being loops of their own:
    # blocks the layout placed out of line
    back = [(a, b) for a, b in loops if fa <= a < ta and tb < b <= fb and not any(
        r[0] <= a and b <= r[1] and r[1] - r[0] < b - a and r != (a, b) for r in ranges)]
    if back:
        print(f"  out-of-line blocks behind the trip loop that branch back into the set-up: {len(back)} branches, "
              f"sources [{min(b for _, b in back)}, {max(b for _, b in back)}]")
    tail = [seq[i] for i in range(fb + 1, len(seq)) if src[i] == "chunk end"]
    print(f"  chunk end (output rows, WriteCommon, state stores) {fmt(tail)}")
    cold = [seq[i] for i in range(len(seq)) if src[i] == "reset branch"]
    print(f"  reset branch (mt19937 draws; placed behind the loop) {fmt(cold)}")


def check(a, b):
    def instrs(path):
        out = {}
        for name, body in kernels(open(path).read()):
            out[name] = [l.strip() for l in body.split("\n") if l.startswith("\t") and not l.strip().startswith((".", ";"))]
        return out
    x, y = instrs(a), instrs(b)
    bad = [k for k in x if x[k] != y.get(k)]
    print("same instructions in every kernel" if not bad else f"differ: {bad}")
    return 1 if bad else 0


def main():
    if sys.argv[1] == "--check":
        sys.exit(check(sys.argv[2], sys.argv[3]))
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "envpool_amd", "csrc")
    if sys.argv[1] == "--src":
        src = sys.argv[2]
        del sys.argv[1:3]
    txt = open(sys.argv[1]).read()
    files = {int(m.group(1)): os.path.basename(m.group(2)) for m in
             re.finditer(r'\.file\s+(\d+)\s+"[^"]*"\s+"([^"]+)"', txt)}
    segs = segments(src)
    want = {k: k for k in sys.argv[2:]} if len(sys.argv) > 2 else KERNELS
    for label, sub in want.items():
        for name, body in kernels(txt):
            if sub in name:
                report(label, *parse(body, files, segs))


if __name__ == "__main__":
    main()
