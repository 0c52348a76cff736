// PGX trainer: what a training step of the built-in nets does around the forward and the backward (pgx_trainer.hip.h is
// the contract; DESIGN.md "PGX trainer").  Five kernels and the handle that owns their memory.
//
// How the work is split.
// TrainerGather: a wave per minibatch row.  The wave computes the row's sample index once and moves the sample's obs
//   bytes, mask bytes, policy row and value into the step's contiguous inputs, 16 bytes per lane and turn where the
//   two addresses and the row size allow, else 4 bytes, else single bytes.
// TrainerLoss: a block of 256 threads takes kTrainerLossRows = 32 rows, eight lanes a row.  The rows' p, pi and mask
//   are contiguous in memory: they enter LDS as three flat copies in 16-byte loads (4-byte and byte loads for an
//   unaligned caller and the tail).  The order-free work is spread over a row's eight lanes, a = lane, lane + 8, ..:
//   the logits and their maximum (three xor shuffles), the exponentials (GumbelExp is most of the arithmetic) and at
//   the end the gradients.  The three sums the contract orders, S, T and U, are each walked in ascending a by ONE lane --
//   lanes 0, 1 and 2 of the row at the same time -- over the values in LDS, and handed to the others by shuffles: the
//   bits are those of the sequential loop, and the sequential part costs A additions, not A exponentials.  dp leaves
//   LDS as one flat copy in 16-byte stores; thread 0 adds the 32 rows' losses in double: the block's partial.
// TrainerNorm: a block per chunk of 1024 gradients, one 16-byte load per thread, squares in double, a tree in LDS.
// TrainerTail: one block.  Three waves add, each in ascending order, the policy-loss partials, the value-loss partials
//   and the norm partials; thread 0 writes the statistics row and the step's clip scale.
// TrainerUpdate: a block per chunk over the one flat space of all parameter arrays (weights first, then biases, each
//   padded to whole chunks, so a chunk never straddles two arrays and needs no table lookup).  A thread owns four
//   elements: one 16-byte load of the gradient, two each of the master and of every state word, the update in double,
//   16-byte stores back and, by the same thread, the quantised values -- four int8 as one 4-byte store for a weight,
//   four int32 as one 16-byte store for a bias.  No scratch: the four elements stay in registers.
//
// All launches of a call are enqueued from one C++ function on the caller's stream; nothing waits.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "engine.h"
#include "pgx_conv.hip.h"
#include "pgx_trainer.hip.h"

namespace epa {
namespace {

constexpr int kRows = pgx::kTrainerLossRows, kGroup = 8;
constexpr int kChunk = pgx::kTrainerChunk;
static_assert(kRows * kGroup == 256 && kChunk == 4 * 256, "the block shapes of the contract");

// A flat copy of `bytes` bytes by the block's 256 threads (by `n` threads from `t` on): 16 bytes a turn where both
// addresses allow, the rest in 4-byte or single-byte turns.
__device__ inline void FlatCopy(void* dst, const void* src, size_t bytes, int t, int n) {
  const uintptr_t both = reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(src);
  size_t done = 0;
  if ((both & 15) == 0) {
    const size_t q = bytes / 16;
    for (size_t i = t; i < q; i += n) static_cast<uint4*>(dst)[i] = static_cast<const uint4*>(src)[i];
    done = q * 16;
  }
  if ((both & 3) == 0) {
    const size_t q = (bytes - done) / 4;
    uint32_t* d = reinterpret_cast<uint32_t*>(static_cast<char*>(dst) + done);
    const uint32_t* s = reinterpret_cast<const uint32_t*>(static_cast<const char*>(src) + done);
    for (size_t i = t; i < q; i += n) d[i] = s[i];
    done += q * 4;
  }
  for (size_t i = done + t; i < bytes; i += n) static_cast<char*>(dst)[i] = static_cast<const char*>(src)[i];
}

// ---------------------------------------------------------------------------
// TrainerGather
// ---------------------------------------------------------------------------
struct GatherArgs {
  int rows, F, A;
  uint32_t t, count;
  uint64_t seed;
  const unsigned char* obs;
  const unsigned char* mask;
  const float* policy;
  const float* value;
  unsigned char* out_obs;
  unsigned char* out_mask;
  float* out_policy;
  float* out_value;
};

__global__ __launch_bounds__(256) void TrainerGather(GatherArgs a) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= a.rows) return;
  const size_t idx = pgx::TrainerIndex(a.seed, a.t, (uint32_t)row, a.count);
  FlatCopy(a.out_obs + (size_t)row * a.F, a.obs + idx * a.F, (size_t)a.F, lane, 64);
  FlatCopy(a.out_mask + (size_t)row * a.A, a.mask + idx * a.A, (size_t)a.A, lane, 64);
  FlatCopy(a.out_policy + (size_t)row * a.A, a.policy + idx * a.A, (size_t)a.A * 4, lane, 64);
  if (lane == 0) a.out_value[row] = a.value[idx];
}

// ---------------------------------------------------------------------------
// TrainerLoss
// ---------------------------------------------------------------------------
struct LossArgs {
  int rows, A;
  float scale_p, scale_v, value_weight;
  const int32_t* p;
  const unsigned char* mask;
  const float* pi;
  const float* z;
  float* dp;
  double* partial;  // [blocks][2]
};

__global__ __launch_bounds__(256) void TrainerLoss(LossArgs a) {
  __shared__ __attribute__((aligned(16))) int32_t s_p[kRows * 128];  // p, then the bits of the logits, then of dp
  __shared__ __attribute__((aligned(16))) float s_pi[kRows * 128];
  __shared__ __attribute__((aligned(16))) float s_e[kRows * 128];
  __shared__ __attribute__((aligned(16))) unsigned char s_mask[kRows * 128];
  __shared__ double s_loss[kRows * 2];
  const int A = a.A, t = threadIdx.x;
  const int r0 = blockIdx.x * kRows;
  const int nr = a.rows - r0 < kRows ? a.rows - r0 : kRows;
  FlatCopy(s_p, a.p + (size_t)r0 * (A + 1), (size_t)nr * (A + 1) * 4, t, 256);
  FlatCopy(s_pi, a.pi + (size_t)r0 * A, (size_t)nr * A * 4, t, 256);
  FlatCopy(s_mask, a.mask + (size_t)r0 * A, (size_t)nr * A, t, 256);
  __syncthreads();

  const int row = t >> 3, l = t & (kGroup - 1), base = (t & 63) & ~(kGroup - 1);
  const bool active = row < nr;
  int32_t* p = s_p + row * (A + 1);
  const float* pi = s_pi + row * A;
  float* e = s_e + row * A;
  const unsigned char* mask = s_mask + row * A;
  const float nf = (float)a.rows;

  float m = -FLT_MAX;
  int any = 0;
  if (active) {
    for (int k = l; k < A; k += kGroup) {
      const float logit = pgx::NetLogit(p[k], a.scale_p);
      p[k] = pgx::NetFloatBits(logit);
      if (mask[k] != 0) {
        any = 1;
        m = logit > m ? logit : m;
      }
    }
  }
  for (int w = kGroup / 2; w >= 1; w >>= 1) {
    const float other = __shfl_xor(m, w);
    m = other > m ? other : m;
    any |= __shfl_xor(any, w);
  }
  if (active) {
    for (int k = l; k < A; k += kGroup) e[k] = mask[k] != 0 ? pgx::GumbelExp(pgx::NetBitsFloat(p[k]) - m) : 0.0f;
  }
  __syncthreads();

  // the ordered sums: lane 0 walks S, lane 1 T, lane 2 U
  float sum = 0.0f;
  if (active && l < 3) {
    for (int k = 0; k < A; ++k) {
      if (mask[k] == 0) continue;
      const float term = l == 0 ? e[k] : (l == 1 ? pi[k] : pi[k] * pgx::NetBitsFloat(p[k]));
      sum = sum + term;
    }
  }
  const float S = __shfl(sum, base), T = __shfl(sum, base + 1), U = __shfl(sum, base + 2);
  __syncthreads();
  if (active) {
    for (int k = l; k < A; k += kGroup) {
      p[k] = pgx::NetFloatBits(mask[k] != 0 ? pgx::TrainerPolicyGrad(a.scale_p, T, e[k], S, pi[k], nf) : 0.0f);
    }
    if (l == 0) {
      const float v = (float)p[A] * a.scale_v, z = a.z[r0 + row];
      p[A] = pgx::NetFloatBits(pgx::TrainerValueGrad(a.value_weight, a.scale_v, v, z, nf));
      s_loss[2 * row] = any ? (double)pgx::TrainerPolicyLoss(T, m, S, U) : 0.0;
      s_loss[2 * row + 1] = (double)pgx::TrainerValueLoss(a.value_weight, v, z);
    }
  }
  __syncthreads();
  FlatCopy(a.dp + (size_t)r0 * (A + 1), s_p, (size_t)nr * (A + 1) * 4, t, 256);
  if (t == 0) {
    double lp = 0.0, lv = 0.0;
    for (int r = 0; r < nr; ++r) {
      lp = lp + s_loss[2 * r];
      lv = lv + s_loss[2 * r + 1];
    }
    a.partial[2 * blockIdx.x] = lp;
    a.partial[2 * blockIdx.x + 1] = lv;
  }
}

// ---------------------------------------------------------------------------
// TrainerNorm, TrainerTail
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void TrainerNorm(const float* __restrict__ grad, double* __restrict__ partial) {
  __shared__ double s[256];
  const int t = threadIdx.x;
  const float4 g = reinterpret_cast<const float4*>(grad + (size_t)blockIdx.x * kChunk)[t];
  double x = 0.0;
  x = x + (double)g.x * (double)g.x;
  x = x + (double)g.y * (double)g.y;
  x = x + (double)g.z * (double)g.z;
  x = x + (double)g.w * (double)g.w;
  s[t] = x;
  __syncthreads();
  for (int w = 128; w >= 1; w >>= 1) {
    if (t < w) s[t] = s[t] + s[t + w];
    __syncthreads();
  }
  if (t == 0) partial[blockIdx.x] = s[0];
}

struct TailArgs {
  int rows, loss_blocks, chunks;
  double clip;
  const double* loss_partial;
  const double* norm_partial;
  double* stats;       // this step's row
  double* clip_scale;  // [1]
};

__global__ __launch_bounds__(256) void TrainerTail(TailArgs a) {
  __shared__ double s[3];
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0 && wave < 3) {
    double x = 0.0;
    if (wave < 2) {
      for (int i = 0; i < a.loss_blocks; ++i) x = x + a.loss_partial[2 * i + wave];
    } else {
      for (int i = 0; i < a.chunks; ++i) x = x + a.norm_partial[i];
    }
    s[wave] = x;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double n = (double)a.rows, norm = sqrt(s[2]);
    a.stats[0] = s[0] / n;
    a.stats[1] = s[1] / n;
    a.stats[2] = norm;
    a.stats[3] = n;
    *a.clip_scale = pgx::TrainerClipScale(a.clip, norm);
  }
}

// ---------------------------------------------------------------------------
// TrainerUpdate
// ---------------------------------------------------------------------------
struct UpdateArgs {
  pgx::TrainerRule rule;
  int weight_chunks;  // the chunks below this one hold weights
  const float* grad;
  double* master;
  double* s1;
  double* s2;
  const double* clip_scale;
  signed char* q_weight;  // one byte per element of the weight chunks
  int32_t* q_bias;        // one word per element of the others
};

__global__ __launch_bounds__(256) void TrainerUpdate(UpdateArgs a) {
  const size_t at = (size_t)blockIdx.x * kChunk + 4 * threadIdx.x;
  const bool adam = a.rule.optimizer == pgx::kTrainerAdam;
  const double clip_scale = *a.clip_scale;
  const float4 g4 = *reinterpret_cast<const float4*>(a.grad + at);
  const float g[4] = {g4.x, g4.y, g4.z, g4.w};
  double2* pm = reinterpret_cast<double2*>(a.master + at);
  double2* p1 = reinterpret_cast<double2*>(a.s1 + at);
  double2* p2 = reinterpret_cast<double2*>(a.s2 + at);
  const double2 m01 = pm[0], m23 = pm[1], a01 = p1[0], a23 = p1[1];
  double2 b01 = make_double2(0.0, 0.0), b23 = b01;
  if (adam) b01 = p2[0], b23 = p2[1];
  double m[4] = {m01.x, m01.y, m23.x, m23.y}, s1[4] = {a01.x, a01.y, a23.x, a23.y};
  double s2[4] = {b01.x, b01.y, b23.x, b23.y};
#pragma unroll
  for (int q = 0; q < 4; ++q) pgx::TrainerUpdateOne(a.rule, g[q], clip_scale, &m[q], &s1[q], &s2[q]);
  pm[0] = make_double2(m[0], m[1]), pm[1] = make_double2(m[2], m[3]);
  p1[0] = make_double2(s1[0], s1[1]), p1[1] = make_double2(s1[2], s1[3]);
  if (adam) p2[0] = make_double2(s2[0], s2[1]), p2[1] = make_double2(s2[2], s2[3]);
  if ((int)blockIdx.x < a.weight_chunks) {
    uint32_t packed = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) packed |= ((uint32_t)pgx::TrainerQuantWeight(m[q]) & 0xffu) << (8 * q);
    *reinterpret_cast<uint32_t*>(a.q_weight + at) = packed;
  } else {
    const size_t b = at - (size_t)a.weight_chunks * kChunk;
    *reinterpret_cast<int4*>(a.q_bias + b) = make_int4(pgx::TrainerQuantBias(m[0]), pgx::TrainerQuantBias(m[1]),
                                                       pgx::TrainerQuantBias(m[2]), pgx::TrainerQuantBias(m[3]));
  }
}

size_t Align256(size_t n) { return (n + 255) & ~(size_t)255; }

void CheckOption(const char* name, double v) {
  if (!(v >= 0.0) || !std::isfinite(v)) {
    throw std::invalid_argument(std::string("trainer_create: ") + name + " = " + std::to_string(v) +
                                " must be finite and not negative");
  }
}

}  // namespace

// the launches the PPO trainer shares (engine.h)
void TrainerNormLaunch(const float* grad, int chunks, double* partial, hipStream_t stream) {
  hipLaunchKernelGGL(TrainerNorm, dim3(chunks), dim3(256), 0, stream, grad, partial);
}

void TrainerUpdateLaunch(const pgx::TrainerRule& rule, int chunks, int weight_chunks, const float* grad, double* master,
                         double* s1, double* s2, const double* clip_scale, signed char* q_weight, int32_t* q_bias,
                         hipStream_t stream) {
  const UpdateArgs up{rule, weight_chunks, grad, master, s1, s2, clip_scale, q_weight, q_bias};
  hipLaunchKernelGGL(TrainerUpdate, dim3(chunks), dim3(256), 0, stream, up);
}

// ---------------------------------------------------------------------------
// the handle (engine.h: Trainer)
// ---------------------------------------------------------------------------
struct Trainer::Layout {
  int arrays{0};
  size_t count[2 * kConvImageLayers]{}, eoff[2 * kConvImageLayers]{};  // elements and the flat offset of an array
  size_t elems{0}, weight_elems{0};                                     // of the flat space, all whole chunks
  // byte offsets into the block
  size_t grad, master, s1, s2, q_weight, q_bias, dp, p, obs, mask, policy, value, loss_partial, norm_partial, clip,
      stats, total;
};

Trainer::Trainer(int device, const void* blob, size_t bytes, const TrainerOptions& o, long long max_rows)
    : device_(device), max_rows_((int)max_rows), opt_(o), at_(new Layout()) {
  if (o.optimizer != pgx::kTrainerSgd && o.optimizer != pgx::kTrainerAdam) {
    throw std::invalid_argument("trainer_create: optimizer = " + std::to_string(o.optimizer) +
                                " must be 0 (sgd) or 1 (adam)");
  }
  CheckOption("lr", o.lr), CheckOption("momentum", o.momentum), CheckOption("beta1", o.beta1);
  CheckOption("beta2", o.beta2), CheckOption("eps", o.eps), CheckOption("weight_decay", o.weight_decay);
  CheckOption("value_weight", o.value_weight), CheckOption("clip", o.clip);
  if (max_rows < 1 || max_rows > (1 << 22)) {
    throw std::invalid_argument("trainer_create: max_rows = " + std::to_string(max_rows) + " must be 1 .. 2^22");
  }
  char err[240];
  std::vector<const signed char*> w;
  std::vector<const int32_t*> b;
  Layout& at = *at_;
  conv_ = ConvIsBlob(blob, bytes);
  pgx::NetView nv{};
  pgx::ConvView cv{};
  if (conv_) {
    if (!pgx::ConvParse(blob, bytes, &cv, err, sizeof(err))) throw std::invalid_argument(err);
    layers_ = cv.layers(), F_ = cv.H * cv.W * cv.C, A_ = cv.A, scale_p_ = cv.scale_p, scale_v_ = cv.scale_v;
    for (int i = 0; i < layers_; ++i) {
      const pgx::ConvLayer& l = cv.layer[i];
      at.count[i] = (size_t)l.n_out * l.taps * l.k_in, at.count[layers_ + i] = (size_t)l.n_out;
      w.push_back(l.w), b.push_back(l.b), shift_[i] = l.shift;
    }
    cnn_.reset(new ConvTrain(device, cv.H, cv.W, cv.C, cv.A, cv.D, cv.L, cv.P, max_rows));
  } else {
    if (!pgx::NetParse(blob, bytes, &nv, err, sizeof(err))) throw std::invalid_argument(err);
    layers_ = nv.layers(), F_ = nv.F, A_ = nv.A, scale_p_ = nv.scale_p, scale_v_ = nv.scale_v;
    for (int i = 0; i < layers_; ++i) {
      const pgx::NetLayer& l = nv.layer[i];
      at.count[i] = (size_t)l.n_out * l.k_in, at.count[layers_ + i] = (size_t)l.n_out;
      w.push_back(l.w), b.push_back(l.b), shift_[i] = l.shift;
    }
    net_.reset(new NetTrain(device, nv.F, nv.A, nv.D, nv.L, max_rows));
  }
  at.arrays = 2 * layers_;
  for (int s = 0; s < at.arrays; ++s) {
    at.eoff[s] = at.elems;
    at.elems += (at.count[s] + kChunk - 1) / kChunk * kChunk;
    if (s == layers_ - 1) at.weight_elems = at.elems;
  }
  const size_t rows = (size_t)max_rows_, E = at.elems, A1 = (size_t)A_ + 1;
  size_t end = 0;
  auto take = [&](size_t n) {
    const size_t here = end;
    end += Align256(n);
    return here;
  };
  at.grad = take(4 * E), at.master = take(8 * E), at.s1 = take(8 * E), at.s2 = take(8 * E);
  at.q_weight = take(at.weight_elems), at.q_bias = take(4 * (E - at.weight_elems));
  at.dp = take(rows * A1 * 4), at.p = take(rows * A1 * 4);
  at.obs = take(rows * F_), at.mask = take(rows * A_), at.policy = take(rows * A_ * 4), at.value = take(rows * 4);
  at.loss_partial = take((rows + kRows - 1) / kRows * 16), at.norm_partial = take(E / kChunk * 8);
  at.clip = take(8), at.stats = take((size_t)pgx::kTrainerStatRows * 32);
  at.total = end;

  // the start: masters = the blob's integers, their quantised arrays, everything else zero
  std::vector<double> master(E, 0.0);
  std::vector<signed char> qw(at.weight_elems, 0);
  std::vector<int32_t> qb(E - at.weight_elems, 0);
  for (int i = 0; i < layers_; ++i) {
    for (size_t k = 0; k < at.count[i]; ++k) master[at.eoff[i] + k] = (double)(qw[at.eoff[i] + k] = w[i][k]);
    const size_t bo = at.eoff[layers_ + i];
    for (size_t k = 0; k < at.count[layers_ + i]; ++k) master[bo + k] = (double)(qb[bo - at.weight_elems + k] = b[i][k]);
  }
  int before = 0;
  EPA_HIP(hipGetDevice(&before));
  EPA_HIP(hipSetDevice(device_));
  try {
    mem_.Alloc(at.total);
    EPA_HIP(hipMemset(mem_.p, 0, at.total));
    EPA_HIP(hipMemcpy(mem_.p + at.master, master.data(), 8 * E, hipMemcpyHostToDevice));
    EPA_HIP(hipMemcpy(mem_.p + at.q_weight, qw.data(), qw.size(), hipMemcpyHostToDevice));
    EPA_HIP(hipMemcpy(mem_.p + at.q_bias, qb.data(), 4 * qb.size(), hipMemcpyHostToDevice));
    EPA_HIP(hipDeviceSynchronize());
  } catch (...) {
    (void)hipSetDevice(before);
    throw;
  }
  EPA_HIP(hipSetDevice(before));
}

Trainer::~Trainer() {
  int before = 0;
  if (hipGetDevice(&before) != hipSuccess) return;
  (void)hipSetDevice(device_);
  mem_.Free();
  net_.reset(), cnn_.reset();
  (void)hipSetDevice(before);
}

void Trainer::Enqueue(hipStream_t stream, int rows, const unsigned char* obs, const unsigned char* mask,
                      const float* policy, const float* value) {
  const Layout& at = *at_;
  char* m = mem_.p;
  const void* qw[kConvImageLayers];
  const void* qb[kConvImageLayers];
  void* dw[kConvImageLayers];
  void* db[kConvImageLayers];
  float* grad = reinterpret_cast<float*>(m + at.grad);
  for (int i = 0; i < layers_; ++i) {
    qw[i] = m + at.q_weight + at.eoff[i];
    qb[i] = m + at.q_bias + 4 * (at.eoff[layers_ + i] - at.weight_elems);
    dw[i] = grad + at.eoff[i];
    db[i] = grad + at.eoff[layers_ + i];
  }
  int32_t* p = reinterpret_cast<int32_t*>(m + at.p);
  float* dp = reinterpret_cast<float*>(m + at.dp);
  if (conv_) {
    cnn_->Forward(stream, rows, qw, qb, shift_, obs, p);
  } else {
    net_->Forward(stream, rows, qw, qb, shift_, obs, p);
  }
  const int loss_blocks = (rows + kRows - 1) / kRows, chunks = (int)(at.elems / kChunk);
  double* loss_partial = reinterpret_cast<double*>(m + at.loss_partial);
  double* norm_partial = reinterpret_cast<double*>(m + at.norm_partial);
  double* clip_scale = reinterpret_cast<double*>(m + at.clip);
  int before = 0;
  EPA_HIP(hipGetDevice(&before));
  EPA_HIP(hipSetDevice(device_));
  const LossArgs loss{rows, A_, scale_p_, scale_v_, (float)opt_.value_weight, p, mask, policy, value, dp, loss_partial};
  hipLaunchKernelGGL(TrainerLoss, dim3(loss_blocks), dim3(256), 0, stream, loss);
  hipError_t launched = hipGetLastError();
  (void)hipSetDevice(before);
  EPA_HIP(launched);
  if (conv_) {
    cnn_->Backward(stream, rows, dp, dw, db);
  } else {
    net_->Backward(stream, rows, dp, dw, db);
  }
  // the step's constants, in the host's doubles
  beta1_pow_ *= opt_.beta1, beta2_pow_ *= opt_.beta2;
  pgx::TrainerRule rule{};
  rule.optimizer = opt_.optimizer, rule.lr = opt_.lr, rule.momentum = opt_.momentum;
  rule.beta1 = opt_.beta1, rule.beta2 = opt_.beta2, rule.eps = opt_.eps, rule.weight_decay = opt_.weight_decay;
  rule.one_minus_beta1 = 1.0 - opt_.beta1, rule.one_minus_beta2 = 1.0 - opt_.beta2;
  rule.lr_t = opt_.optimizer == pgx::kTrainerAdam ? opt_.lr * std::sqrt(1.0 - beta2_pow_) / (1.0 - beta1_pow_) : 0.0;
  double* stats = reinterpret_cast<double*>(m + at.stats) + 4 * (size_t)(steps_ % pgx::kTrainerStatRows);
  const TailArgs tail{rows, loss_blocks, chunks, opt_.clip, loss_partial, norm_partial, stats, clip_scale};
  const UpdateArgs up{rule,
                      (int)(at.weight_elems / kChunk),
                      grad,
                      reinterpret_cast<double*>(m + at.master),
                      reinterpret_cast<double*>(m + at.s1),
                      reinterpret_cast<double*>(m + at.s2),
                      clip_scale,
                      reinterpret_cast<signed char*>(m + at.q_weight),
                      reinterpret_cast<int32_t*>(m + at.q_bias)};
  EPA_HIP(hipSetDevice(device_));
  hipLaunchKernelGGL(TrainerNorm, dim3(chunks), dim3(256), 0, stream, grad, norm_partial);
  hipLaunchKernelGGL(TrainerTail, dim3(1), dim3(256), 0, stream, tail);
  hipLaunchKernelGGL(TrainerUpdate, dim3(chunks), dim3(256), 0, stream, up);
  launched = hipGetLastError();
  (void)hipSetDevice(before);
  EPA_HIP(launched);
  ++steps_, rows_ = rows, last_ = stream;
}

void Trainer::Step(hipStream_t stream, int rows, const void* d_obs, const void* d_mask, const void* d_policy,
                   const void* d_value) {
  if (d_obs == nullptr || d_mask == nullptr || d_policy == nullptr || d_value == nullptr) {
    throw std::invalid_argument("trainer_step: null argument");
  }
  if (rows < 1 || rows > max_rows_) {
    throw std::invalid_argument("trainer_step: rows = " + std::to_string(rows) + " must be 1 .. " +
                                std::to_string(max_rows_) + " (the handle's max_rows)");
  }
  Enqueue(stream, rows, static_cast<const unsigned char*>(d_obs), static_cast<const unsigned char*>(d_mask),
          static_cast<const float*>(d_policy), static_cast<const float*>(d_value));
}

void Trainer::Fit(hipStream_t stream, const void* const* arrays, long long count, int batch, int steps) {
  if (arrays == nullptr || arrays[0] == nullptr || arrays[1] == nullptr || arrays[2] == nullptr ||
      arrays[3] == nullptr) {
    throw std::invalid_argument("trainer_fit: null argument");
  }
  if (batch < 1 || batch > max_rows_) {
    throw std::invalid_argument("trainer_fit: batch = " + std::to_string(batch) + " must be 1 .. " +
                                std::to_string(max_rows_) + " (the handle's max_rows)");
  }
  if (count < 1 || count > 0xffffffffll) {
    throw std::invalid_argument("trainer_fit: count = " + std::to_string(count) + " must be 1 .. 2^32 - 1");
  }
  if (steps < 1) throw std::invalid_argument("trainer_fit: steps = " + std::to_string(steps) + " must be at least 1");
  const Layout& at = *at_;
  GatherArgs g{batch, F_, A_, 0, (uint32_t)count, opt_.seed,
               static_cast<const unsigned char*>(arrays[0]), static_cast<const unsigned char*>(arrays[1]),
               static_cast<const float*>(arrays[2]), static_cast<const float*>(arrays[3]),
               reinterpret_cast<unsigned char*>(mem_.p + at.obs), reinterpret_cast<unsigned char*>(mem_.p + at.mask),
               reinterpret_cast<float*>(mem_.p + at.policy), reinterpret_cast<float*>(mem_.p + at.value)};
  for (int s = 0; s < steps; ++s) {
    g.t = (uint32_t)steps_;
    int before = 0;
    EPA_HIP(hipGetDevice(&before));
    EPA_HIP(hipSetDevice(device_));
    hipLaunchKernelGGL(TrainerGather, dim3((batch + 3) / 4), dim3(256), 0, stream, g);
    const hipError_t launched = hipGetLastError();
    (void)hipSetDevice(before);
    EPA_HIP(launched);
    Enqueue(stream, batch, g.out_obs, g.out_mask, g.out_policy, g.out_value);
  }
}

void Trainer::Read(int what, int layer, void* out) {
  const Layout& at = *at_;
  size_t from = 0, bytes = 0;
  const bool array = what >= 0 && what <= 4;
  if ((array || what == 8) && (layer < 0 || layer >= at.arrays)) {
    throw std::invalid_argument("trainer_read: layer = " + std::to_string(layer) + " must be 0 .. " +
                                std::to_string(at.arrays - 1));
  }
  if (what == 8) {
    const int64_t info[4] = {at.arrays, steps_, rows_, (int64_t)at.count[layer]};
    std::memcpy(out, info, sizeof(info));
    return;
  }
  if (array) {
    const size_t e = at.eoff[layer], n = at.count[layer];
    const bool weight = layer < layers_;
    if (what <= 2) {
      from = (what == 0 ? at.master : (what == 1 ? at.s1 : at.s2)) + 8 * e, bytes = 8 * n;
    } else if (what == 3) {
      from = weight ? at.q_weight + e : at.q_bias + 4 * (e - at.weight_elems), bytes = weight ? n : 4 * n;
    } else {
      from = at.grad + 4 * e, bytes = 4 * n;
    }
  } else if (what == 5 || what == 6) {
    from = what == 5 ? at.dp : at.p, bytes = (size_t)rows_ * (A_ + 1) * 4;
  } else if (what == 7) {
    if (layer < 0 || layer > pgx::kTrainerStatRows || layer > steps_) {
      throw std::invalid_argument("trainer_read: " + std::to_string(layer) + " statistics rows; there are " +
                                  std::to_string(steps_ < pgx::kTrainerStatRows ? steps_ : pgx::kTrainerStatRows));
    }
  } else {
    throw std::invalid_argument("trainer_read: what = " + std::to_string(what) + " must be 0 .. 8");
  }
  int before = 0;
  EPA_HIP(hipGetDevice(&before));
  EPA_HIP(hipSetDevice(device_));
  hipError_t e = hipStreamSynchronize(last_);
  if (e == hipSuccess && what == 7) {
    for (int i = 0; i < layer && e == hipSuccess; ++i) {  // (the ring: row by row)
      const size_t slot = (size_t)((steps_ - layer + i) % pgx::kTrainerStatRows);
      e = hipMemcpy(static_cast<char*>(out) + 32 * (size_t)i, mem_.p + at.stats + 32 * slot, 32, hipMemcpyDeviceToHost);
    }
  } else if (e == hipSuccess && bytes != 0) {
    e = hipMemcpy(out, mem_.p + from, bytes, hipMemcpyDeviceToHost);
  }
  (void)hipSetDevice(before);
  EPA_HIP(e);
}

}  // namespace epa
