// Jumanji board puzzles: RenderableEnv::Render of envpool/jumanji/*_env.h over the drawing rules of
// envpool/jumanji/render_utils.h, as __host__ __device__ code on a render::Canvas.  Shared by the render kernel
// (jumanji.hip) and the g++ host harness of the tests (tests/cpu_harness/render_host.cpp); byte-identical with
// the reference for every state and size.
//
// What is kept on purpose:
//   - the primitives come in the reference's order (the canvas keeps later ones on top);
//   - DrawNumber draws a value >= 100 as its last digit only (DrawDigit refuses the "digit" value / 10 > 9), and
//     DrawDigit draws nothing into a box narrower than 4 or lower than 6;
//   - StrokeRect's four runs are independent: a box with right <= left still gets its two vertical runs, at
//     `left` and at `right - 1` (RubiksCube with face_side 1 paints left of its stickers that way);
//   - Blend's colours are tables made on the host with the reference's own float expression (Game2048 exponents
//     3..11, constant from 11 on; SlidingTilePuzzle tiles 0..25): nothing is rounded on the device.
#ifndef ENVPOOL_AMD_CSRC_JUMANJI_RENDER_HIP_H_
#define ENVPOOL_AMD_CSRC_JUMANJI_RENDER_HIP_H_

#include "jumanji_env.hip.h"
#include "render_canvas.hip.h"

namespace epa {
namespace jm {

using render::Canvas;
using render::Color;

// render_utils.h ------------------------------------------------------------------------------------------------
JM_HD inline void StrokeRect(Canvas& cv, int left, int top, int right, int bottom, Color c, int thickness = 1) {
  for (int i = 0; i < thickness; ++i) {
    cv.Rect(left + i, top + i, right - i, top + i + 1, c);
    cv.Rect(left + i, bottom - 1 - i, right - i, bottom - i, c);
    cv.Rect(left + i, top + i, left + i + 1, bottom - i, c);
    cv.Rect(right - 1 - i, top + i, right - i, bottom - i, c);
  }
}

JM_HD inline void FillCell(Canvas& cv, int rows, int cols, int row, int col, Color c, int pad = 0) {
  const int left = col * cv.W / cols, right = (col + 1) * cv.W / cols;
  const int top = row * cv.H / rows, bottom = (row + 1) * cv.H / rows;
  cv.Rect(left + pad, top + pad, right - pad, bottom - pad, c);
}

JM_HD inline void DrawGrid(Canvas& cv, int rows, int cols, Color c, int thickness = 1) {
  for (int row = 0; row <= rows; ++row) {
    const int y = row * cv.H / rows;
    cv.Rect(0, y - thickness / 2, cv.W, y + (thickness + 1) / 2, c);
  }
  for (int col = 0; col <= cols; ++col) {
    const int x = col * cv.W / cols;
    cv.Rect(x - thickness / 2, 0, x + (thickness + 1) / 2, cv.H, c);
  }
}

JM_HD inline void CellCenter(const Canvas& cv, int rows, int cols, int row, int col, int* x, int* y) {
  const int x0 = col * cv.W / cols, x1 = (col + 1) * cv.W / cols;
  const int y0 = row * cv.H / rows, y1 = (row + 1) * cv.H / rows;
  *x = (x0 + x1) / 2;
  *y = (y0 + y1) / 2;
}

JM_HD inline Color Palette(int index) {
  const Color colors[20] = {{31, 119, 180},  {255, 127, 14},  {44, 160, 44},   {214, 39, 40},   {148, 103, 189},
                            {140, 86, 75},   {227, 119, 194}, {127, 127, 127}, {188, 189, 34},  {23, 190, 207},
                            {174, 199, 232}, {255, 187, 120}, {152, 223, 138}, {255, 152, 150}, {197, 176, 213},
                            {196, 156, 148}, {247, 182, 210}, {199, 199, 199}, {219, 219, 141}, {158, 218, 229}};
  return colors[((index % 20) + 20) % 20];
}

JM_HD inline void DrawDigit(Canvas& cv, int digit, int left, int top, int right, int bottom, Color c) {
  if (digit < 0 || digit > 9 || right - left < 4 || bottom - top < 6) return;
  const uint8_t segments[10] = {0x7e, 0x30, 0x6d, 0x79, 0x33, 0x5b, 0x5f, 0x70, 0x7f, 0x7b};
  const int w = right - left, h = bottom - top;
  const int t = render::Max(1, render::Min(w, h) / 7);
  const int mid = top + h / 2;
  const uint8_t s = segments[digit];
  if (s & 0x40) cv.Rect(left + t, top, right - t, top + t, c);
  if (s & 0x20) cv.Rect(right - t, top + t, right, mid, c);
  if (s & 0x10) cv.Rect(right - t, mid, right, bottom - t, c);
  if (s & 0x08) cv.Rect(left + t, bottom - t, right - t, bottom, c);
  if (s & 0x04) cv.Rect(left, mid, left + t, bottom - t, c);
  if (s & 0x02) cv.Rect(left, top + t, left + t, mid, c);
  if (s & 0x01) cv.Rect(left + t, mid - t / 2, right - t, mid + (t + 1) / 2, c);
}

JM_HD inline void DrawNumber(Canvas& cv, int value, int left, int top, int right, int bottom, Color c) {
  if (value < 0) return;
  if (value < 10) {
    DrawDigit(cv, value, left, top, right, bottom, c);
    return;
  }
  const int mid = (left + right) / 2;
  DrawDigit(cv, value / 10, left, top, mid - 1, bottom, c);
  DrawDigit(cv, value % 10, mid + 1, top, right, bottom, c);
}

// Blend({242,177,121}, {237,94,66}, min(1, (value - 3) / 8.0f)) for value = 3..11
JM_HD inline Color Game2048Blend(int value) {
  const Color t[9] = {{242, 177, 121}, {241, 167, 114}, {241, 156, 107}, {240, 146, 100}, {240, 136, 94},
                      {239, 125, 87},  {238, 115, 80},  {238, 104, 73},  {237, 94, 66}};
  return t[render::Min(value, 11) - 3];
}
// Blend({224,228,255}, {36,74,235}, tile / 25.0f) for tile = 0..25 (t clamps to [0, 1] outside)
JM_HD inline Color SlidingTileBlend(int tile) {
  const Color t[26] = {{224, 228, 255}, {216, 222, 254}, {209, 216, 253}, {201, 210, 253}, {194, 203, 252},
                       {186, 197, 251}, {179, 191, 250}, {171, 185, 249}, {164, 179, 249}, {156, 173, 248},
                       {149, 166, 247}, {141, 160, 246}, {134, 154, 245}, {126, 148, 245}, {119, 142, 244},
                       {111, 136, 243}, {104, 129, 242}, {96, 123, 241},  {89, 117, 241},  {81, 111, 240},
                       {74, 105, 239},  {66, 99, 238},   {59, 92, 237},   {51, 86, 237},   {44, 80, 236},
                       {36, 74, 235}};
  return t[render::Max(0, render::Min(tile, 25))];
}

// XxxEnv::Render ------------------------------------------------------------------------------------------------
JM_HD inline void Render(Canvas& cv, const Game2048State& s) {
  cv.Clear({187, 173, 160});
  for (int row = 0; row < 4; ++row) {
    for (int col = 0; col < 4; ++col) {
      const int value = s.board[row * 4 + col];
      const int left = col * cv.W / 4 + 3, right = (col + 1) * cv.W / 4 - 3;
      const int top = row * cv.H / 4 + 3, bottom = (row + 1) * cv.H / 4 - 3;
      Color color = {205, 193, 180};
      if (value == 1) {
        color = {238, 228, 218};
      } else if (value == 2) {
        color = {237, 224, 200};
      } else if (value > 2) {
        color = Game2048Blend(value);
      }
      cv.Rect(left, top, right, bottom, color);
      // (a 4 x 4 board tops out at exponent 17; the shift is kept defined for any word set_state wrote)
      if (value > 0) DrawNumber(cv, 1 << render::Min(value, 30), left + 8, top + 8, right - 8, bottom - 8, {90, 80, 70});
    }
  }
}

JM_HD inline void Render(Canvas& cv, const MinesweeperState& s) {
  cv.Clear({255, 255, 255});
  for (int row = 0; row < 10; ++row) {
    for (int col = 0; col < 10; ++col) {
      const int value = s.board[row * 10 + col];
      Color color = {206, 206, 206};
      if (value >= 0) color = {246, 246, 246};
      FillCell(cv, 10, 10, row, col, color, 1);
      if (value > 0) {
        const int left = col * cv.W / 10, right = (col + 1) * cv.W / 10;
        const int top = row * cv.H / 10, bottom = (row + 1) * cv.H / 10;
        DrawNumber(cv, value, left + 6, top + 5, right - 6, bottom - 5, Palette(value));
      }
    }
  }
  DrawGrid(cv, 10, 10, {150, 150, 150});
}

JM_HD inline void Render(Canvas& cv, const SlidingTileState& s) {
  cv.Clear({255, 255, 255});
  for (int row = 0; row < 5; ++row) {
    for (int col = 0; col < 5; ++col) {
      const int tile = s.puzzle[row * 5 + col];
      const int left = col * cv.W / 5, right = (col + 1) * cv.W / 5;
      const int top = row * cv.H / 5, bottom = (row + 1) * cv.H / 5;
      if (tile == 0) {
        cv.Rect(left + 1, top + 1, right - 1, bottom - 1, {48, 54, 61});
      } else {
        cv.Rect(left + 1, top + 1, right - 1, bottom - 1, SlidingTileBlend(tile));
        DrawNumber(cv, tile, left + 7, top + 7, right - 7, bottom - 7, {25, 25, 40});
      }
    }
  }
  DrawGrid(cv, 5, 5, {150, 150, 150});
}

JM_HD inline void Render(Canvas& cv, const RubiksCubeState& s) {
  cv.Clear({255, 255, 255});
  const Color colors[6] = {{255, 255, 255}, {255, 214, 0}, {0, 82, 255}, {0, 155, 72}, {255, 88, 0}, {183, 18, 52}};
  const int face_pos[6][2] = {{1, 0}, {0, 1}, {1, 1}, {2, 1}, {3, 1}, {1, 2}};
  const int face_side = render::Max(1, render::Min(cv.W / 4, cv.H / 3) - 4);
  const int x_origin = (cv.W - 4 * face_side) / 2;
  const int y_origin = (cv.H - 3 * face_side) / 2;
  for (int face = 0; face < 6; ++face) {
    const int face_left = x_origin + face_pos[face][0] * face_side;
    const int face_top = y_origin + face_pos[face][1] * face_side;
    for (int row = 0; row < 3; ++row) {
      for (int col = 0; col < 3; ++col) {
        // (a sticker is 0..5 in every state the env reaches; any other byte set_state wrote stays inside the table)
        const int value = render::Min((int)(uint8_t)s.cube[face * 9 + row * 3 + col], 5);
        const int left = face_left + col * face_side / 3, right = face_left + (col + 1) * face_side / 3;
        const int top = face_top + row * face_side / 3, bottom = face_top + (row + 1) * face_side / 3;
        cv.Rect(left + 1, top + 1, right - 1, bottom - 1, colors[value]);
        StrokeRect(cv, left, top, right, bottom, {0, 0, 0});
      }
    }
  }
}

JM_HD inline void Render(Canvas& cv, const SnakeState& s) {
  cv.Clear({255, 255, 255});
  StrokeRect(cv, 0, 0, cv.W, cv.H, {170, 170, 170});
  for (int row = 0; row < 12; ++row) {
    for (int col = 0; col < 12; ++col) {
      if (s.body[row * 12 + col] > 0) FillCell(cv, 12, 12, row, col, {40, 170, 40}, 2);
    }
  }
  int x, y;
  CellCenter(cv, 12, 12, s.fruit_row, s.fruit_col, &x, &y);
  cv.Rect(x - 4, y - 4, x + 5, y + 5, {65, 180, 40});
  CellCenter(cv, 12, 12, s.head_row, s.head_col, &x, &y);
  cv.Disc(x, y, render::Max(3, render::Min(cv.W, cv.H) / 40), {220, 50, 50});
}

JM_HD inline void Render(Canvas& cv, const MazeState& s) {
  cv.Clear({255, 255, 255});
  for (int row = 0; row < 10; ++row) {
    for (int col = 0; col < 10; ++col) {
      const Color color = s.walls[row * 10 + col] ? Color{0, 0, 0} : Color{255, 255, 255};
      FillCell(cv, 10, 10, row, col, color);
    }
  }
  DrawGrid(cv, 10, 10, {210, 210, 210});
  int x, y;
  CellCenter(cv, 10, 10, s.target_row, s.target_col, &x, &y);
  cv.Rect(x - 5, y - 5, x + 6, y + 6, {0, 210, 70});
  CellCenter(cv, 10, 10, s.agent_row, s.agent_col, &x, &y);
  cv.Disc(x, y, render::Max(3, render::Min(cv.W, cv.H) / 40), {220, 30, 30});
}

// RenderSize: every puzzle defaults to 256 x 256
JM_HD inline void RenderSize(int width, int height, int* w, int* h) {
  *w = width > 0 ? width : 256;
  *h = height > 0 ? height : 256;
}

}  // namespace jm
}  // namespace epa

#endif  // ENVPOOL_AMD_CSRC_JUMANJI_RENDER_HIP_H_
