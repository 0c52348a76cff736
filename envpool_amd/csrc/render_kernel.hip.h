// The render kernel of the board families (jumanji.hip, pgx.hip): uint8 [k, H, W, 3] frames of the listed envs,
// painted from their persistent state by the family's painter (jumanji_render.hip.h, pgx_render.hip.h).
//
// A frame does not fit LDS (256 x 256 x 3 = 192 KB), so it is cut into bands of whole rows, at most kBandBytes
// each, one workgroup per (frame, band): a default 256 x 256 frame is 16 workgroups, a 16 x 16 one is 1.  The
// workgroup is one wave: it paints its band in LDS in the reference's painter's order, every primitive clipped
// to the band (render_canvas.hip.h: a single wave's LDS stores land in program order, so no barrier is needed
// between primitives), and then streams the band out.  The band's bytes are contiguous in the frame, so they go
// as 16-byte words, with the bytes before the first and after the last 16-byte boundary one by one (pgx.hip's
// EmitKey is the model).  The band sits in LDS at the same offset from a 16-byte boundary as its first byte in
// HBM, so both sides of a word copy are aligned, whatever the caller's base pointer and 3 * W are.
#ifndef ENVPOOL_AMD_CSRC_RENDER_KERNEL_HIP_H_
#define ENVPOOL_AMD_CSRC_RENDER_KERNEL_HIP_H_

#include <hip/hip_runtime.h>

#include <algorithm>
#include <stdexcept>
#include <string>

#include "engine.h"
#include "render_canvas.hip.h"

namespace epa {
namespace render {

constexpr int kBlock = kWave;  // one wave per workgroup: painter's order without barriers (render_canvas.hip.h)
constexpr int kBandBytes = 12 * 1024;  // 13 one-wave workgroups per CU by LDS; a row of kMaxSide pixels just fits

struct Launch {
  int w, h, rows, bands;  // rows per band, bands per frame
};

// width / height as RenderSize resolved them
inline Launch Plan(int w, int h, int k) {
  if (w <= 0 || h <= 0) throw std::invalid_argument("resolved render width and height must be positive");
  if (w > kMaxSide || h > kMaxSide) {
    throw std::invalid_argument("render: a frame side above " + std::to_string(kMaxSide) + " is not supported");
  }
  Launch l{w, h, 0, 0};
  const int fit = std::max(1, kBandBytes / (3 * w));
  l.bands = (h + fit - 1) / fit;
  l.rows = (h + l.bands - 1) / l.bands;  // even bands
  l.bands = (h + l.rows - 1) / l.rows;
  if ((long long)l.bands * k > 0x7fffffffLL) throw std::invalid_argument("render: too many frames for one launch");
  return l;
}

// P: struct { using State = ...; static __device__ void Paint(Canvas&, const State&); }
template <class P>
__global__ __launch_bounds__(kBlock) void RenderKernel(const typename P::State* __restrict__ st,
                                                       const int* __restrict__ ids, Launch l,
                                                       uint8_t* __restrict__ out) {
  extern __shared__ uint4 band_lds[];
  const int frame = blockIdx.x / l.bands, band = blockIdx.x - frame * l.bands;
  const int y0 = band * l.rows, y1 = min(l.h, y0 + l.rows);
  const size_t row_bytes = (size_t)3 * l.w;
  uint8_t* g = out + ((size_t)frame * l.h + y0) * row_bytes;
  const int mis = (int)((uintptr_t)g & 15);
  uint8_t* b = reinterpret_cast<uint8_t*>(band_lds) + mis;
  Canvas cv(b, l.w, l.h, y0, y1);
  P::Paint(cv, st[ids[frame]]);
  cv.Finish();
  const int total = (y1 - y0) * (int)row_bytes;
  const int head = min(total, (16 - mis) & 15);
  const int words = (total - head) / 16;
  const int tail = head + words * 16;
  for (int i = threadIdx.x; i < head; i += kBlock) g[i] = b[i];
  for (int c = threadIdx.x; c < words; c += kBlock) {
    *reinterpret_cast<uint4*>(g + head + (size_t)c * 16) = *reinterpret_cast<const uint4*>(b + head + (size_t)c * 16);
  }
  for (int i = tail + threadIdx.x; i < total; i += kBlock) g[i] = b[i];
}

// d_ids: local env ids [k]; d_rgb: uint8 [k, h, w, 3], any alignment
template <class P>
void LaunchRender(const typename P::State* st, const int* d_ids, int k, int w, int h, void* d_rgb,
                  hipStream_t stream) {
  const Launch l = Plan(w, h, k);
  const size_t lds = (size_t)l.rows * 3 * w + 16;
  hipLaunchKernelGGL(RenderKernel<P>, dim3((unsigned)(l.bands * k)), dim3(kBlock), lds, stream, st, d_ids, l,
                     static_cast<uint8_t*>(d_rgb));
  EPA_HIP(hipGetLastError());
}

}  // namespace render
}  // namespace epa

#endif  // ENVPOOL_AMD_CSRC_RENDER_KERNEL_HIP_H_
