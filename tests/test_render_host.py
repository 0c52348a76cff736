"""Board rendering, CPU side: the painting rules of the render kernels (envpool_amd/csrc/jumanji_render.hip.h,
pgx_render.hip.h on render_canvas.hip.h) built for the host by g++ -Wall -Werror and compared byte for byte with
the frames the reference's own Render painted (tests/golden/render_*.npz), at every fixture size; RenderSize's
defaults; Blend's colours read back from the tile interiors; and what the fixtures cover."""
import numpy as np
import pytest

from render_util import GAMES, SIZES, build_harness, fixture, host_paint, host_size, tags


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_harness(tmp_path_factory.mktemp("render"))


@pytest.mark.parametrize("game", sorted(GAMES))
def test_host_paint_matches_reference_frames(harness, game):
    g = fixture(game)
    assert [tuple(s) for s in g["sizes"]] == SIZES
    for s, (w, h) in enumerate(g["resolved"]):
        want = g[f"frame_{s}"]
        assert want.shape == (len(g["hidden"]), h, w, 3) and want.dtype == np.uint8
        for p, words in enumerate(g["hidden"]):
            got = host_paint(harness, game, words, int(w), int(h))
            assert np.array_equal(got, want[p]), (game, (int(w), int(h)), p)


@pytest.mark.parametrize("game", sorted(GAMES))
@pytest.mark.parametrize("band", [1, 5, 32])
def test_host_paint_in_bands_is_the_same_frame(harness, game, band):
    """The kernel paints a frame as row bands, one workgroup each: every band repeats the primitives clipped to
    its own rows, and the bands together are the frame."""
    g = fixture(game)
    for s, (w, h) in enumerate(g["resolved"]):
        for p, words in enumerate(g["hidden"]):
            got = host_paint(harness, game, words, int(w), int(h), band=band)
            assert np.array_equal(got, g[f"frame_{s}"][p]), (game, (int(w), int(h)), p, band)


@pytest.mark.parametrize("game", sorted(GAMES))
def test_render_size_defaults(harness, game):
    dw, dh = GAMES[game][3]
    assert host_size(harness, game, 0, 0) == (dw, dh)
    assert host_size(harness, game, -1, -7) == (dw, dh)
    assert host_size(harness, game, 61, 0) == (61, dh)
    assert host_size(harness, game, 0, 45) == (dw, 45)
    assert host_size(harness, game, 61, 45) == (61, 45)
    assert tuple(fixture(game)["resolved"][0]) == (dw, dh)


def _interior(frame, rows, cols, row, col):
    """A pixel inside the tile of cell (row, col) and off its number: five pixels in from the cell's corner."""
    h, w = frame.shape[:2]
    return tuple(int(v) for v in frame[row * h // rows + 5, col * w // cols + 5])


def test_blend_colours_of_every_game2048_exponent(harness):
    """Exponents 3..15 (t = min(1, (e - 3) / 8)): the colour the reference's frame shows inside the tile, and
    the same from the host paint.  A board that holds 0..15 is part of the fixture."""
    g = fixture("Game2048")
    p = [i for i, t in enumerate(tags("Game2048")) if "exponents_0_to_15" in t][0]
    board = g["hidden"][p][:16]
    ref = g["frame_0"][p]
    mine = host_paint(harness, "Game2048", g["hidden"][p], 256, 256)
    seen = {}
    for cell, e in enumerate(board):
        if e >= 3:
            seen[int(e)] = _interior(ref, 4, 4, cell // 4, cell % 4)
            assert _interior(mine, 4, 4, cell // 4, cell % 4) == seen[int(e)], e
    assert sorted(seen) == list(range(3, 16))
    for e, c in seen.items():  # between the two end colours, and constant from exponent 11 on
        t = min(1.0, (e - 3) / 8.0)
        exact = [a * (1 - t) + b * t for a, b in zip((242, 177, 121), (237, 94, 66))]
        assert all(abs(x - y) <= 0.5 + 1e-3 for x, y in zip(c, exact)), (e, c)
        if e >= 11:
            assert c == (237, 94, 66)


def test_blend_colours_of_every_sliding_tile(harness):
    g = fixture("SlidingTilePuzzle")
    seen = {}
    for p, words in enumerate(g["hidden"]):
        ref = g["frame_0"][p]
        mine = host_paint(harness, "SlidingTilePuzzle", words, 256, 256)
        for cell, tile in enumerate(words[:25]):
            c = _interior(ref, 5, 5, cell // 5, cell % 5)
            assert _interior(mine, 5, 5, cell // 5, cell % 5) == c
            if tile > 0:
                assert seen.setdefault(int(tile), c) == c
            else:
                assert c == (48, 54, 61)
    assert sorted(seen) == list(range(1, 25))
    for tile, c in seen.items():
        t = tile / 25.0
        exact = [a * (1 - t) + b * t for a, b in zip((224, 228, 255), (36, 74, 235))]
        assert all(abs(x - y) <= 0.5 + 1e-3 for x, y in zip(c, exact)), (tile, c)


def test_fixtures_cover_the_quirks():
    want = {"Game2048": {"exponents_0_to_15", "rolled_out"},
            "Minesweeper": {"unexplored", "zero", "count1", "count2", "count3"},
            "SlidingTilePuzzle": {"scrambled"}, "RubiksCube": {"six_colours_in_one_row"},
            "Snake": {"length4", "head_on_border", "head_next_to_fruit"},
            "Maze": {"walls", "agent_on_border", "agent_next_to_target"},
            "TicTacToe": {"both_colours", "adjacent"}, "ConnectFour": {"both_colours", "adjacent"},
            "Hex": {"both_colours", "adjacent", "last_cell"}, "Othello": {"both_colours", "adjacent"}}
    for game in GAMES:
        assert set().union(*map(set, tags(game))) >= want[game], game
    # a 128 tile shows its last digit only: its left half-box stays the tile's colour
    g = fixture("Game2048")
    p = [i for i, t in enumerate(tags("Game2048")) if "exponents_0_to_15" in t][0]
    cell = int(np.where(g["hidden"][p][:16] == 7)[0][0])
    row, col = divmod(cell, 4)
    frame = g["frame_0"][p]
    left, right, top, bottom = col * 64 + 3 + 8, (col + 1) * 64 - 3 - 8, row * 64 + 3 + 8, (row + 1) * 64 - 3 - 8
    mid = (left + right) // 2
    ink = (frame[top:bottom, left:right] == (90, 80, 70)).all(axis=-1)
    assert not ink[:, :mid + 1 - left].any() and ink[:, mid + 1 - left:].any()
    # Hex's last cell clips at the right edge of the default frame: its disc would reach past column 351
    hexg = fixture("Hex")
    p = [i for i, t in enumerate(tags("Hex")) if "last_cell" in t][0]
    assert 10 * 352 // 11 + 352 // 22 + 10 * 352 // 180 + 352 // 36 >= 352
    edge = hexg["frame_0"][p][:, 351]
    stone = (edge == (35, 35, 35)).all(axis=-1) | (edge == (220, 60, 60)).all(axis=-1)
    assert stone[320:].sum() == 17  # the last board row: |dx| = 4 of a radius-9 disc centred on column 355
