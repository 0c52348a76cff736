"""CPU checks of the Atari post-process references (no GPU).

1. tests/atari_post_ref.py (NumPy stack, palette, planes, four flags) agrees with the older
   `OraclePost` (oracle/atari/atari_post.c's own stack) where both apply: gray, no palette,
   flags 0 / 1, on the sequence of test_post_process_bit_exact_with_resets_and_partial_ids.
2. How far the restated cv::resize (UNPINNED: OpenCV is not available to pin it) can be from the
   mathematical resize: `orc_resize_area_u8` against the exact area average and
   `orc_resize_linear_u8` against exact bilinear sampling at (d + 0.5) * scale - 0.5 with clamped
   edges, both in float64.  The bound of 1 grey level is derived, not measured: float32
   accumulation of at most 36 products of values <= 255 errs far below 0.5; the 11-bit linear
   coefficients err by at most 255 * 2 / 2048 ~ 0.25 before the final rounding; so only the
   rounding of a near-tie can come out on the other side.  The share of such pixels is printed
   per case (pytest -s), not asserted; DESIGN.md records it.
"""
import numpy as np
import pytest

from atari_post_ref import RefPost, resize, scripted_sequence

SIZES = [  # (raw, out): the shapes of tests/test_gpu_atari_post_forms.py
    ((210, 160), (84, 84)), ((210, 160), (64, 64)), ((210, 160), (40, 30)), ((210, 160), (96, 75)),
    ((210, 160), (83, 84)), ((210, 160), (45, 44)), ((210, 160), (85, 85)), ((96, 80), (41, 33)),
    ((240, 244), (100, 100)),
]


def area_weights(ssize, dsize):
    """W[d, s] = the share of destination cell d that source pixel s covers."""
    scale = ssize / dsize
    lo = np.arange(dsize)[:, None] * scale
    s = np.arange(ssize)[None, :]
    overlap = np.minimum(lo + scale, s + 1) - np.maximum(lo, s)
    return np.clip(overlap, 0, None) / scale


def linear_weights(ssize, dsize):
    f = (np.arange(dsize) + 0.5) * (ssize / dsize) - 0.5
    i0 = np.floor(f).astype(int)
    t = f - i0
    w = np.zeros((dsize, ssize))
    np.add.at(w, (np.arange(dsize), np.clip(i0, 0, ssize - 1)), 1 - t)
    np.add.at(w, (np.arange(dsize), np.clip(i0 + 1, 0, ssize - 1)), t)
    return w


def inputs(raw):
    rng = np.random.default_rng(raw[0] * 1000 + raw[1])
    return {
        "random": rng.integers(0, 256, raw, dtype=np.uint8),
        "two_level": (rng.integers(0, 2, raw) * 255).astype(np.uint8),
        "constant": np.full(raw, 131, np.uint8),
    }


@pytest.mark.parametrize("linear", [False, True], ids=["area", "linear"])
@pytest.mark.parametrize("raw,out", SIZES, ids=[f"{r[0]}x{r[1]}-{o[0]}x{o[1]}" for r, o in SIZES])
def test_restated_resize_within_one_level_of_exact(raw, out, linear):
    weights = linear_weights if linear else area_weights
    wy, wx = weights(raw[0], out[0]), weights(raw[1], out[1])
    np.testing.assert_allclose(wy.sum(1), 1, atol=1e-12)
    np.testing.assert_allclose(wx.sum(1), 1, atol=1e-12)
    for name, src in inputs(raw).items():
        exact = np.rint(wy @ src.astype(np.float64) @ wx.T).astype(int)
        got = resize(src, *out, linear=linear).astype(int)
        diff = np.abs(got - exact)
        print(f"{'linear' if linear else 'area'} {raw[0]}x{raw[1]}->{out[0]}x{out[1]} {name}: "
              f"{100 * (diff != 0).mean():.2f} % of pixels differ, max {diff.max()}")
        assert diff.max() <= 1, name
        if name == "constant":
            assert (got == 131).all()


def test_ref_post_equals_oracle_post_on_the_existing_sequence():
    from test_gpu_atari_post import OraclePost, pong_like

    n = 64
    ref, orc = RefPost(n), OraclePost(n)
    rng = np.random.default_rng(0)
    ids = np.arange(n, dtype=np.int32)
    frames, mask = pong_like(rng, n), np.ones(n, np.uint8)
    np.testing.assert_array_equal(ref.push(frames, ids, mask), orc.push(frames, ids, mask))
    for t in range(12):
        if t % 3 == 2:
            sub = rng.permutation(n)[:17].astype(np.int32)
            frames = rng.integers(0, 256, (17, 2, 210, 160), dtype=np.uint8)
            mask = (rng.random(17) < 0.3).astype(np.uint8)
        else:
            sub, frames, mask = ids, pong_like(rng, n), None
        np.testing.assert_array_equal(ref.push(frames, sub, mask), orc.push(frames, sub, mask), err_msg=f"push {t}")


def test_ref_post_flags_planes_and_layout():
    """The reference's own stack handling on a case small enough to state by hand."""
    pal = np.stack([np.arange(256), 255 - np.arange(256), np.arange(256) // 2]).astype(np.uint8)
    ref = RefPost(1, s=3, oh=84, ow=84, gray=False, palette=pal)

    def frame(v0, v1):
        f = np.empty((1, 2, 210, 160), np.uint8)
        f[0, 0], f[0, 1] = v0, v1
        return f

    def slots(obs):  # [slot][plane] -> the constant value of every plane
        assert (obs == obs[..., :1, :1]).all()
        return obs[0, :, 0, 0].reshape(3, 3).tolist()

    assert slots(ref.push(frame(10, 200), mask=np.array([1], np.uint8))) == [[10, 245, 5]] * 3  # frame 0 only
    # lookup before the max: plane 1 takes the SMALLER index
    assert slots(ref.push(frame(20, 40))) == [[10, 245, 5], [10, 245, 5], [40, 235, 20]]
    assert slots(ref.push(frame(60, 250), mask=np.array([2], np.uint8))) == [[10, 245, 5], [40, 235, 20], [60, 195, 30]]
    assert slots(ref.push(frame(1, 1), mask=np.array([4], np.uint8))) == [[40, 235, 20], [60, 195, 30], [60, 195, 30]]
    assert ref.heads().tolist() == [0]
    assert slots(ref.push(frame(7, 9))) == [[60, 195, 30], [60, 195, 30], [9, 248, 4]]
    assert ref.heads().tolist() == [1]


def test_scripted_sequence_holds_what_the_gpu_tests_rely_on():
    n = 8
    seq, diverged = scripted_sequence(np.random.default_rng(1), n)
    assert len(seq) >= 12
    masks = [np.zeros(len(ids), np.uint8) if m is None else m for _, ids, m in seq]
    assert (masks[0] == 1).all() and len(seq[0][1]) == n
    assert any(set(m.tolist()) == {0, 1, 2, 4} for m in masks)
    full = [t for t, (_, ids, _) in enumerate(seq) if len(ids) == n and (ids == np.arange(n)).all()]
    assert any(t in full and t + 1 in full and ((masks[t] == 1) & (masks[t + 1] == 4)).any() for t in range(len(seq) - 1))
    assert any(t in full and t + 1 in full and ((masks[t] == 4) & (masks[t + 1] == 4)).any() for t in range(len(seq) - 1))
    ids = seq[diverged][1]
    assert len(ids) < n and len(set(ids.tolist())) == len(ids)
    assert 1 not in masks[diverged].tolist()  # no fill: every pushed env's head moves by one
