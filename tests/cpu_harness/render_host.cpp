// TEST HARNESS (not product): host instantiation of envpool_amd/csrc/jumanji_render.hip.h and pgx_render.hip.h,
// built with g++ by tests/test_render_host.py and compared with the frames the reference's own Render painted
// (tests/golden/render_*.npz).  A state is given as the hidden words get_state reports after (elapsed step,
// done).  Not linked by envpool_amd/.
#include <cstdint>
#include <cstring>

#include "../../envpool_amd/csrc/jumanji_render.hip.h"
#include "../../envpool_amd/csrc/pgx_render.hip.h"

using epa::render::Canvas;

namespace {

// the frame band by band, `band` rows each (<= 0: one band), like the kernel's workgroups paint it
template <class S, class F>
void Bands(const S& s, int w, int h, int band, uint8_t* rgb, F paint) {
  if (band <= 0) band = h;
  for (int y0 = 0; y0 < h; y0 += band) {
    Canvas cv(rgb + (size_t)y0 * 3 * w, w, h, y0, y0 + band < h ? y0 + band : h);
    paint(cv, s);
    cv.Finish();
  }
}

template <int P>
int Jumanji(const int32_t* words, int w, int h, int band, uint8_t* rgb) {
  typename epa::jm::State<P>::T s;
  std::memset(&s, 0, sizeof(s));
  if (!epa::jm::SetHiddenP<P>(s, words)) return -2;
  Bands(s, w, h, band, rgb, [](Canvas& cv, const typename epa::jm::State<P>::T& st) { epa::jm::Render(cv, st); });
  return 0;
}

template <int G>
int Pgx(const int32_t* words, int w, int h, int band, uint8_t* rgb) {
  epa::pgx::State s{};
  if (!epa::pgx::SetHidden<G>(s, words)) return -2;
  Bands(s, w, h, band, rgb, [](Canvas& cv, const epa::pgx::State& st) { epa::pgx::Render<G>(cv, st); });
  return 0;
}

}  // namespace

extern "C" {

// family 0: Jumanji (game = epa::jm::Puzzle), 1: PGX (game = epa::pgx::Game).  rgb: uint8 [h, w, 3], every byte
// of it written.  0, -1 for an unknown game, -2 for words that are no state.
int render_paint(int family, int game, const int32_t* words, int w, int h, int band, uint8_t* rgb) {
  if (family == 0) {
    switch (game) {
      case epa::jm::kGame2048: return Jumanji<epa::jm::kGame2048>(words, w, h, band, rgb);
      case epa::jm::kMinesweeper: return Jumanji<epa::jm::kMinesweeper>(words, w, h, band, rgb);
      case epa::jm::kSlidingTile: return Jumanji<epa::jm::kSlidingTile>(words, w, h, band, rgb);
      case epa::jm::kRubiksCube: return Jumanji<epa::jm::kRubiksCube>(words, w, h, band, rgb);
      case epa::jm::kSnake: return Jumanji<epa::jm::kSnake>(words, w, h, band, rgb);
      case epa::jm::kMaze: return Jumanji<epa::jm::kMaze>(words, w, h, band, rgb);
      default: return -1;
    }
  }
  switch (game) {
    case epa::pgx::kTicTacToe: return Pgx<epa::pgx::kTicTacToe>(words, w, h, band, rgb);
    case epa::pgx::kConnectFour: return Pgx<epa::pgx::kConnectFour>(words, w, h, band, rgb);
    case epa::pgx::kHex: return Pgx<epa::pgx::kHex>(words, w, h, band, rgb);
    case epa::pgx::kOthello: return Pgx<epa::pgx::kOthello>(words, w, h, band, rgb);
    default: return -1;
  }
}

// RenderSize of the game: a width or height <= 0 is its default
int render_size(int family, int game, int width, int height, int* w, int* h) {
  if (family == 0) {
    if (game < 0 || game > epa::jm::kMaze) return -1;
    epa::jm::RenderSize(width, height, w, h);
    return 0;
  }
  switch (game) {
    case epa::pgx::kTicTacToe: epa::pgx::RenderSize<epa::pgx::kTicTacToe>(width, height, w, h); return 0;
    case epa::pgx::kConnectFour: epa::pgx::RenderSize<epa::pgx::kConnectFour>(width, height, w, h); return 0;
    case epa::pgx::kHex: epa::pgx::RenderSize<epa::pgx::kHex>(width, height, w, h); return 0;
    case epa::pgx::kOthello: epa::pgx::RenderSize<epa::pgx::kOthello>(width, height, w, h); return 0;
    default: return -1;
  }
}

}  // extern "C"
