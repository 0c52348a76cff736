// The canvas the board renderers (jumanji_render.hip.h, pgx_render.hip.h) paint on: a band of rows of one
// uint8 [H, W, 3] frame, painted in the reference's painter's order (later primitives overwrite earlier ones).
// __host__ __device__ code, shared by the render kernel (render_kernel.hip.h) and the g++ host harness of the
// tests (tests/cpu_harness/render_host.cpp).
//
// On the device the band lives in LDS and the workgroup is ONE wave, which paints each primitive together: lane i
// takes pixels i, i + 64, ... of the primitive's clipped rectangle in row-major order, whatever its shape (a
// grid line one pixel wide keeps 64 lanes busy).  Painter's order then needs no barrier: the LDS stores of a wave
// are issued and performed in program order, so where two primitives touch the same pixel the later one's
// store lands last, from whichever lanes the two come.
// On the host one "lane" walks every pixel.
//
// Every primitive is a rectangle clipped to the frame, optionally with a per-pixel test (a disc).  The
// reference's two FillRect flavours (Jumanji clamps the corners into the frame, PGX tests every pixel against
// it) paint the same pixels: the rectangle's intersection with the frame.
#ifndef ENVPOOL_AMD_CSRC_RENDER_CANVAS_HIP_H_
#define ENVPOOL_AMD_CSRC_RENDER_CANVAS_HIP_H_

#include <cstdint>

#if defined(__HIPCC__)
#define RN_HD __host__ __device__
#else
#define RN_HD
#endif

namespace epa {
namespace render {

struct Color {
  uint8_t r, g, b;
};

RN_HD inline int Min(int a, int b) { return a < b ? a : b; }
RN_HD inline int Max(int a, int b) { return a > b ? a : b; }

// the largest frame side render accepts: a row of 3 * kMaxSide bytes still fits the kernel's LDS band
constexpr int kMaxSide = 4096;
// the kernel's workgroup: one wave (render_kernel.hip.h)
constexpr int kWave = 64;

struct Canvas {
  uint8_t* px;  // byte 0 of row y0
  int W, H;     // the frame
  int y0, y1;   // the band's rows [y0, y1)

  RN_HD Canvas(uint8_t* p, int w, int h, int b0, int b1) : px(p), W(w), H(h), y0(b0), y1(b1) {}

  // pixels (x, y) of [l, r) x [t, b) inside the frame and the band for which in(x, y) holds
  template <class In>
  RN_HD void Paint(int l, int t, int r, int b, Color c, In in) {
    l = Max(l, 0);
    r = Min(r, W);
    t = Max(t, y0);
    b = Min(b, y1);
    if (l >= r || t >= b) return;
    const int w = r - l, n = w * (b - t);
#if defined(__HIP_DEVICE_COMPILE__)
    // lane i takes pixels i, i + 64, ... of the rectangle's row-major order; (x, y) advance without a division
    const int lane = threadIdx.x, step = kWave;
    int y = (int)((float)lane / (float)w);  // lane < 64, w <= kMaxSide: off by one at most
    if (y * w > lane) --y;
    if ((y + 1) * w <= lane) ++y;
    int x = lane - y * w;
    const int ys = step / w, xs = step - ys * w;
#else
    const int lane = 0, step = 1, ys = w == 1 ? 1 : 0, xs = w == 1 ? 0 : 1;
    int x = 0, y = 0;
#endif
    for (int i = lane; i < n; i += step) {
      if (in(l + x, t + y)) {
        uint8_t* p = px + ((size_t)(t + y - y0) * (size_t)W + (size_t)(l + x)) * 3;
        p[0] = c.r;
        p[1] = c.g;
        p[2] = c.b;
      }
      x += xs;
      y += ys;
      if (x >= w) {
        x -= w;
        ++y;
      }
    }
#if defined(__HIP_DEVICE_COMPILE__)
    __builtin_amdgcn_wave_barrier();  // (no instruction: keeps the primitives' stores in program order)
#endif
  }

  RN_HD void Rect(int l, int t, int r, int b, Color c) {
    Paint(l, t, r, b, c, [](int, int) { return true; });
  }
  RN_HD void Clear(Color c) { Rect(0, 0, W, H, c); }
  // FillCircle / DrawCircle: every pixel of the bounding square within `radius` of the centre
  RN_HD void Disc(int cx, int cy, int radius, Color c) {
    const int r2 = radius * radius;
    Paint(cx - radius, cy - radius, cx + radius + 1, cy + radius + 1, c, [=](int x, int y) {
      const int dx = x - cx, dy = y - cy;
      return dx * dx + dy * dy <= r2;
    });
  }
  // after the last primitive: the band is complete for every lane
  RN_HD void Finish() {
#if defined(__HIP_DEVICE_COMPILE__)
    __syncthreads();
#endif
  }
};

}  // namespace render
}  // namespace epa

#endif  // ENVPOOL_AMD_CSRC_RENDER_CANVAS_HIP_H_
