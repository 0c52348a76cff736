"""The Atari post-process kernel (envpool_amd/csrc/atari_post.hip) in every form it is compiled
in, bit for bit against tests/atari_post_ref.py: palette lookup before the max, one or three
planes, the four per-row flags, stack_num 1 / 2 / 4, every store / copy alignment class, the host
path's chunking, the device entry, the pinned frame buffer and the refusals at construction.

Instantiation `AtariPostKernel<XT, YT, kLinear, kChan>` reached by each test id (every form-matrix
case drives flags 0, 1, 2 and 4; `*` = every value of that parameter):

  <3,4,false,1>  test_form_matrix[area84-gray-*], [area84-graypal-*]; test_pinned_frame_buffer
                 test_push_device_matches_reference[gray]
  <3,4,false,3>  test_form_matrix[area84-rgb-*]; test_host_chunking; test_push_device_matches_reference[rgb]
  <6,6,false,1>  test_form_matrix[area64-gray*-*], [area40x30-gray*-*]; test_alignment_classes[*-gray-area]
                 test_raw_size_off_default[gray-area]
  <6,6,false,3>  test_form_matrix[area64-rgb-*], [area40x30-rgb-*]; test_alignment_classes[*-rgb-area]
                 test_largest_accepted_raw_size[area]
  <2,2,true,1>   test_form_matrix[linear84-gray*-*], [linear96x75-gray*-*]; test_byte_max_exhaustive[*]
                 test_alignment_classes[*-gray-linear]
  <2,2,true,3>   test_form_matrix[linear84-rgb-*], [linear96x75-rgb-*]; test_alignment_classes[*-rgb-linear]
                 test_raw_size_off_default[rgb-linear]; test_largest_accepted_raw_size[linear]
stack_num 1 and 4 run for all fifteen (resize, colour) pairs of the form matrix, stack_num 2 for three.
"""
import numpy as np
import pytest

from atari_post_ref import RefPost, random_palette, scripted_sequence
from envpool_amd.atari import AtariPostProcess

pytestmark = pytest.mark.gpu

RESIZES = {  # name -> (img_height, img_width, use_inter_area_resize)
    "area84": (84, 84, True),        # <3,4>
    "area64": (64, 64, True),        # <6,6>, 5 y taps
    "area40x30": (40, 30, True),     # <6,6>, 6 / 6 taps, byte stores
    "linear84": (84, 84, False),
    "linear96x75": (96, 75, False),  # byte stores
}
COLOURS = ("gray", "graypal", "rgb")
FORM_CASES = [(r, c, s) for s in (1, 4) for r in RESIZES for c in COLOURS] + [
    ("area84", "rgb", 2), ("area40x30", "rgb", 2), ("linear96x75", "graypal", 2)]


def make_pair(rng, n, s, oh, ow, area, colour, raw=(210, 160)):
    gray = colour != "rgb"
    pal = None if colour == "gray" else random_palette(rng, gray)
    gpu = AtariPostProcess(n, stack_num=s, img_height=oh, img_width=ow, raw_height=raw[0], raw_width=raw[1],
                           use_inter_area_resize=area, gray_scale=gray, palette=pal)
    ref = RefPost(n, s, oh, ow, raw, linear=not area, gray=gray, palette=pal)
    return gpu, ref, pal


@pytest.mark.parametrize("resize,colour,s", FORM_CASES, ids=[f"{r}-{c}-s{s}" for r, c, s in FORM_CASES])
def test_form_matrix(resize, colour, s):
    oh, ow, area = RESIZES[resize]
    n = 8
    rng = np.random.default_rng(100 + s)
    gpu, ref, pal = make_pair(rng, n, s, oh, ow, area, colour)
    seq, diverged = scripted_sequence(rng, n)
    assert len(seq) >= 12
    if pal is not None:
        # the premise of the palette cases: on this input "max, then lookup" is a different picture
        good = RefPost(n, s, oh, ow, linear=not area, gray=colour != "rgb", palette=pal)
        swapped = RefPost(n, s, oh, ow, linear=not area, gray=colour != "rgb", palette=pal, lookup_first=False)
        frames, ids, _ = seq[1]
        assert not np.array_equal(good.push(frames, ids, None), swapped.push(frames, ids, None))
    seen = set()
    for t, (frames, ids, mask) in enumerate(seq):
        seen |= {0} if mask is None else set(mask.tolist())
        want = ref.push(frames, ids, mask)
        got = gpu.push(frames, ids, mask)
        assert got.shape == (len(ids), s * (1 if colour != "rgb" else 3), oh, ow)
        np.testing.assert_array_equal(got, want, err_msg=f"push {t}")
        if t == diverged and s > 1:
            assert len(set(ref.heads().tolist())) > 1, ref.heads()
    assert seen == {0, 1, 2, 4}
    gpu.close()


@pytest.mark.parametrize("palette", [False, True], ids=["plain", "identity_palette"])
def test_byte_max_exhaustive(palette):
    """Every (a, b) byte pair through the packed max.  INTER_LINEAR 210x160 -> 209x160 has x weights
    (2048, 0), and with all rows of a frame equal every output row is the pooled row:
    (((2048 * (p * 128)) >> 16) + 2) >> 2 == p.  Pixel i = e * 160 + x holds a = i % 256 and
    b = (i // 256 + 64 * (i % 4)) % 256: a bijection onto the pairs over i < 65536, and three of four
    aligned 4-byte words hold both a < b and a > b lanes (the four b of a word are 64 apart)."""
    n = 410
    i = np.arange(n * 160)
    a, b = (i % 256).astype(np.uint8), ((i // 256 + 64 * (i % 4)) % 256).astype(np.uint8)
    pairs = a[:65536].astype(np.int64) * 256 + b[:65536]
    assert len(np.unique(pairs)) == 65536
    words = (a[:65536].reshape(-1, 4).astype(int) - b[:65536].reshape(-1, 4))
    assert ((words < 0).any(axis=1) & (words > 0).any(axis=1)).mean() > 0.7
    p = np.arange(256)
    assert ((((2048 * (p * 128)) >> 16) + 2) >> 2 == p).all()
    frames = np.empty((n, 2, 210, 160), np.uint8)
    frames[:, 0] = a.reshape(n, 1, 160)
    frames[:, 1] = b.reshape(n, 1, 160)
    gpu = AtariPostProcess(n, stack_num=1, img_height=209, img_width=160, use_inter_area_resize=False,
                           palette=np.arange(256, dtype=np.uint8) if palette else None)
    want = np.broadcast_to(np.maximum(a, b).reshape(n, 1, 1, 160), (n, 1, 209, 160))
    np.testing.assert_array_equal(gpu.push(frames), want)
    np.testing.assert_array_equal(gpu.push(frames[:, ::-1]), want)  # max(b, a)
    gpu.close()


FLAGS = np.array([0, 1, 2, 4], np.uint8)


def run_random(gpu, ref, rng, n, raw, pushes=6):
    """Random frames and flags, the first push a reset of every env, one push partial."""
    for t in range(pushes):
        k = n - 3 if t == 3 else n
        ids = rng.permutation(n)[:k].astype(np.int32) if t == 3 else np.arange(n, dtype=np.int32)
        frames = rng.integers(0, 256, (k, 2, *raw), dtype=np.uint8)
        mask = np.ones(k, np.uint8) if t == 0 else FLAGS[rng.integers(0, 4, k)]
        np.testing.assert_array_equal(gpu.push(frames, ids, mask), ref.push(frames, ids, mask), err_msg=f"push {t}")


@pytest.mark.parametrize("area", [True, False], ids=["area", "linear"])
@pytest.mark.parametrize("colour", ["gray", "rgb"])
@pytest.mark.parametrize("oh,ow", [(83, 84), (45, 44), (85, 85)], ids=["83x84", "45x44", "85x85"])
def test_alignment_classes(oh, ow, colour, area):
    """(83, 84), (45, 44): 32-bit stores of the new frame, but a plane of 12 bytes modulo 16, so the
    older frames are copied bytewise (and the RGB planes start at every 4-byte phase);
    (85, 85): byte stores, odd plane size."""
    assert (ow % 4 == 0 and oh * ow % 16 == 12 and 3 * oh * ow % 16 != 0) or ow % 4 == 1
    n = 8
    rng = np.random.default_rng(oh * 1000 + ow)
    gpu, ref, _ = make_pair(rng, n, 3, oh, ow, area, colour)
    run_random(gpu, ref, rng, n, (210, 160))
    gpu.close()


@pytest.mark.parametrize("colour,area", [("gray", True), ("rgb", False)], ids=["gray-area", "rgb-linear"])
def test_raw_size_off_default(colour, area):
    """A raw frame that is not Atari's: 96 x 80 (a multiple of 16 pixels) to 41 x 33."""
    n = 8
    rng = np.random.default_rng(9680)
    gpu, ref, _ = make_pair(rng, n, 4, 41, 33, area, colour, raw=(96, 80))
    run_random(gpu, ref, rng, n, (96, 80))
    gpu.close()


@pytest.mark.parametrize("area", [True, False], ids=["area", "linear"])
def test_largest_accepted_raw_size(area):
    """240 x 244 -> 100 x 100 RGB stages 58560 + 28 * 200 + 768 = 64928 bytes in LDS, the most that
    the constructor accepts for this output (the limit is 65536)."""
    n = 4
    rng = np.random.default_rng(240244)
    gpu, ref, _ = make_pair(rng, n, 2, 100, 100, area, "rgb", raw=(240, 244))
    run_random(gpu, ref, rng, n, (240, 244), pushes=5)
    gpu.close()


def test_host_chunking():
    """Pushes of 64 rows and more go up, through the kernel and down in four chunks whose row
    offsets need not be multiples of 4: k = 67 splits into 16 + 17 + 17 + 17.  k = 63 is the last
    unchunked size."""
    n = 70
    rng = np.random.default_rng(70)
    gpu, ref, _ = make_pair(rng, n, 4, 84, 84, True, "rgb")
    frames = rng.integers(0, 256, (n, 2, 210, 160), dtype=np.uint8)
    ids = np.arange(n, dtype=np.int32)
    np.testing.assert_array_equal(gpu.push(frames, ids, np.ones(n, np.uint8)), ref.push(frames, ids, np.ones(n, np.uint8)))
    for k in (63, 64, 67, 67):
        ids = rng.permutation(n)[:k].astype(np.int32)
        frames = rng.integers(0, 256, (k, 2, 210, 160), dtype=np.uint8)
        mask = FLAGS[rng.integers(0, 4, k)]
        np.testing.assert_array_equal(gpu.push(frames, ids, mask), ref.push(frames, ids, mask), err_msg=f"k {k}")
    gpu.close()


@pytest.mark.parametrize("colour", ["gray", "rgb"])
def test_push_device_matches_reference(colour):
    """The device-resident entry (what tools/bench_atari_post.py and tools/bench_families.py time),
    interleaved with host pushes on the same object: both advance the same ring."""
    import torch

    dev = torch.device("cuda", 0)
    n, s = 8, 4
    rng = np.random.default_rng(17)
    gpu, ref, _ = make_pair(rng, n, s, 84, 84, True, colour)
    planes = s * (1 if colour == "gray" else 3)
    stream = torch.cuda.ExternalStream(gpu.stream, device=dev)
    all_ids = np.arange(n, dtype=np.int32)

    def device_push(frames, ids, mask):
        k = frames.shape[0]
        d_frames = torch.from_numpy(frames).to(dev)
        d_ids = None if ids is None else torch.from_numpy(ids).to(dev)
        d_mask = None if mask is None else torch.from_numpy(mask).to(dev)
        d_obs = torch.zeros((k, planes, 84, 84), device=dev, dtype=torch.uint8)
        torch.cuda.synchronize()  # the uploads ran on torch's stream
        gpu.push_device(d_frames.data_ptr(), d_obs.data_ptr(), k,
                        None if d_ids is None else d_ids.data_ptr(),
                        None if d_mask is None else d_mask.data_ptr())
        stream.synchronize()
        return d_obs.cpu().numpy()

    def frames_of(k):
        return rng.integers(0, 256, (k, 2, 210, 160), dtype=np.uint8)

    steps = [  # (entry, ids, mask)
        ("device", None, np.ones(n, np.uint8)),                    # reset of every env, rows = envs
        ("device", None, None),                                    # no ids, no mask
        ("host", all_ids, None),
        ("device", rng.permutation(n)[:5].astype(np.int32), None),  # ids, no mask
        ("device", rng.permutation(n)[:6].astype(np.int32), np.array([0, 1, 2, 4, 0, 1], np.uint8)),
        ("host", rng.permutation(n)[:5].astype(np.int32), np.array([4, 0, 2, 1, 0], np.uint8)),
        ("device", None, np.resize(FLAGS, n)),                     # mask, no ids
        ("device", all_ids[::-1].copy(), None),
        ("host", all_ids, None),
    ]
    for t, (entry, ids, mask) in enumerate(steps):
        frames = frames_of(n if ids is None else len(ids))
        want = ref.push(frames, ids, mask)
        got = device_push(frames, ids, mask) if entry == "device" else gpu.push(frames, ids, mask)
        np.testing.assert_array_equal(got, want, err_msg=f"step {t} ({entry})")
    gpu.close()


def test_pinned_frame_buffer():
    """Frames written into `frame_buffer()` and pushed from there equal the same frames pushed
    from a pageable array (and the reference)."""
    n = 8
    rng = np.random.default_rng(23)
    pinned, ref, _ = make_pair(rng, n, 4, 84, 84, True, "gray")
    pageable = AtariPostProcess(n)
    fb = pinned.frame_buffer()
    assert fb.shape == (n, 2, 210, 160) and fb.dtype == np.uint8
    assert pinned.frame_buffer() is fb
    for t in range(4):
        k = n if t != 2 else 5
        ids = np.arange(n, dtype=np.int32) if t != 2 else rng.permutation(n)[:k].astype(np.int32)
        frames = rng.integers(0, 256, (k, 2, 210, 160), dtype=np.uint8)
        mask = np.ones(k, np.uint8) if t == 0 else FLAGS[rng.integers(0, 4, k)]
        fb[:k] = frames
        a = pinned.push(fb[:k], ids, mask)
        np.testing.assert_array_equal(a, pageable.push(frames.copy(), ids, mask), err_msg=f"push {t}")
        np.testing.assert_array_equal(a, ref.push(frames, ids, mask), err_msg=f"push {t}")
    pinned.close()
    pageable.close()


def test_refusals():
    """Configurations the kernel cannot run are refused at construction, before any launch."""
    rgb = np.zeros((3, 256), np.uint8)
    with pytest.raises(ValueError):  # 7 taps per axis
        AtariPostProcess(4, img_height=36, img_width=28)
    with pytest.raises(ValueError):  # output larger than the raw frame
        AtariPostProcess(4, img_height=211, img_width=84)
    with pytest.raises(ValueError):
        AtariPostProcess(4, img_height=84, img_width=161, use_inter_area_resize=False)
    with pytest.raises(ValueError):  # RGB needs the palette
        AtariPostProcess(4, gray_scale=False)
    with pytest.raises(ValueError):
        AtariPostProcess(4, stack_num=0)
    # raw frames that 16-byte loads cannot read aligned
    with pytest.raises(ValueError, match="multiple of 16"):
        AtariPostProcess(4, img_height=40, img_width=33, raw_height=97, raw_width=83)
    # more LDS than a launch may ask for: the message gives the number
    with pytest.raises(ValueError, match="66160"):
        AtariPostProcess(4, img_height=100, img_width=100, raw_height=245, raw_width=244, gray_scale=False,
                         palette=rgb)
    with pytest.raises(ValueError, match="65888"):  # the same, with a raw size that is a multiple of 16
        AtariPostProcess(4, img_height=100, img_width=100, raw_height=240, raw_width=248, gray_scale=False,
                         palette=rgb)
    post = AtariPostProcess(4)
    frames = np.zeros((5, 2, 210, 160), np.uint8)
    with pytest.raises(ValueError):  # an id out of range
        post.push(frames[:2], np.array([0, 4], np.int32))
    with pytest.raises(ValueError):
        post.push(frames[:2], np.array([-1, 0], np.int32))
    with pytest.raises(ValueError):  # more rows than envs
        post.push(frames, np.array([0, 1, 2, 3, 0], np.int32))
    # none of the refused pushes moved the stack
    one = np.full((4, 2, 210, 160), 9, np.uint8)
    assert (post.push(one, reset_mask=np.ones(4, np.uint8)) == 9).all()
    post.close()
