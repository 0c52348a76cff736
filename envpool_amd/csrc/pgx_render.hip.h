// PGX board games: XxxEnv::Render of envpool/pgx/board_games.h (DrawGrid, then the stones in cell order as
// DrawCircle) as __host__ __device__ code on a render::Canvas.  Shared by the render kernel (pgx.hip) and the
// g++ host harness of the tests (tests/cpu_harness/render_host.cpp); byte-identical with the reference for
// every state and size.
//
// What is kept on purpose: the stones come in cell order and a later one lies on top (the radii have floors, so
// at small sizes discs overlap each other and the grid lines); Hex shifts the stones of row r right by
// r * width / 180, over their neighbours' cells and off the right edge, where the frame clips them; the grid
// lines are [max(0, p - 1), min(side, p + 1)).
// The stone sets: TicTacToe / ConnectFour a = color 0, b = color 1; Hex / Othello a = board_ > 0, b = board_ < 0.
#ifndef ENVPOOL_AMD_CSRC_PGX_RENDER_HIP_H_
#define ENVPOOL_AMD_CSRC_PGX_RENDER_HIP_H_

#include "pgx_env.hip.h"
#include "render_canvas.hip.h"

namespace epa {
namespace pgx {

using render::Canvas;
using render::Color;

PGX_HD inline void DrawGrid(Canvas& cv, int rows, int cols) {
  cv.Clear({236, 232, 220});
  for (int row = 0; row <= rows; ++row) {
    const int y = row * cv.H / rows;
    cv.Rect(0, render::Max(0, y - 1), cv.W, render::Min(cv.H, y + 1), {70, 70, 70});
  }
  for (int col = 0; col <= cols; ++col) {
    const int x = col * cv.W / cols;
    cv.Rect(render::Max(0, x - 1), 0, render::Min(cv.W, x + 1), cv.H, {70, 70, 70});
  }
}

// RenderSize: width or height <= 0 is the game's default
template <int G>
PGX_HD inline void RenderSize(int width, int height, int* w, int* h) {
  constexpr int dw = G == kTicTacToe ? 192 : G == kConnectFour ? 280 : G == kHex ? 352 : 256;
  constexpr int dh = G == kTicTacToe ? 192 : G == kConnectFour ? 240 : G == kHex ? 352 : 256;
  *w = width > 0 ? width : dw;
  *h = height > 0 ? height : dh;
}

template <int G>
PGX_HD inline void Render(Canvas& cv, const State& s) {
  constexpr int rows = Dims<G>::H, cols = Dims<G>::W;
  const int W = cv.W, H = cv.H;
  DrawGrid(cv, rows, cols);
  int radius;
  Color ca, cb;
  if (G == kTicTacToe) {
    radius = render::Max(4, render::Min(W / cols, H / rows) / 4);
    ca = {30, 30, 30}, cb = {230, 70, 70};
  } else if (G == kConnectFour) {
    radius = render::Max(3, render::Min(W / 7, H / 6) / 3);
    ca = {30, 30, 30}, cb = {220, 60, 60};
  } else if (G == kHex) {
    radius = render::Max(3, render::Min(W, H) / 36);
    ca = {35, 35, 35}, cb = {220, 60, 60};
  } else {
    radius = render::Max(3, render::Min(W, H) / 28);
    ca = {35, 35, 35}, cb = {240, 240, 230};
  }
  for (int i = 0; i < rows * cols; ++i) {
    const bool a = Has(s.a, i);
    if (!a && !Has(s.b, i)) continue;
    const int row = i / cols, col = i % cols;
    int cx = col * W / cols + W / (cols * 2);
    const int cy = row * H / rows + H / (rows * 2);
    if (G == kHex) cx += row * W / 180;
    cv.Disc(cx, cy, radius, a ? ca : cb);
  }
}

}  // namespace pgx
}  // namespace epa

#endif  // ENVPOOL_AMD_CSRC_PGX_RENDER_HIP_H_
