// Internal C++ side of the C ABI in include/envpool_amd.h.
//
// A `Pool` owns: device-resident SoA env state (family specific), a HIP stream
// for the step kernels plus one each for action uploads and result downloads
// (so that in async mode -- several batches in flight, async_envpool.h's whole
// point -- the copies of one batch overlap the kernel of the next, and recv of
// the oldest batch does not wait for work enqueued after it), pinned action
// staging, and a FIFO of result batches.  It replaces
// AsyncEnvPool + ActionBufferQueue + StateBufferQueue of the reference
// (envpool/core/async_envpool.h, action_buffer_queue.h, state_buffer_queue.h):
// "enqueue" = launch one batched step kernel on the stream, "state buffer" = a
// packed device block holding every state key for the k rows of that launch.
#ifndef ENVPOOL_AMD_CSRC_ENGINE_H_
#define ENVPOOL_AMD_CSRC_ENGINE_H_

#include <hip/hip_runtime.h>

#include <climits>
#include <condition_variable>
#include <cstdint>
#include <cstring>
#include <atomic>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "../../include/envpool_amd.h"
#include "rollout.hip.h"

namespace epa {

namespace snap {
struct PoolDesc;  // snapshot.hip.h
}

struct DeviceError : std::runtime_error {
  using std::runtime_error::runtime_error;
};

#define EPA_HIP(expr)                                                        \
  do {                                                                       \
    hipError_t _e = (expr);                                                  \
    if (_e != hipSuccess) {                                                  \
      throw ::epa::DeviceError(std::string(#expr) + ": " +                   \
                               hipGetErrorString(_e));                       \
    }                                                                        \
  } while (0)

inline int DtypeBytes(int dt) {
  switch (dt) {
    case EPA_I32: return 4;
    case EPA_F32: return 4;
    case EPA_F64: return 8;
    default: return 1;
  }
}

struct KeySpec {
  std::string name;
  int dtype;
  std::vector<int> shape;  // per row (= per env); a per-player key's shape starts with the family's player count
  int players{1};          // P of a per-player key ([P, ...] per row: the reference's P player rows), 1 otherwise
  int row_elems() const {
    int n = 1;
    for (int d : shape) n *= d;
    return n;
  }
  int row_bytes() const { return row_elems() * DtypeBytes(dtype); }
};

// Parsed epa_config.
struct Config {
  int num_envs{1};
  int batch_size{0};
  int seed{42};
  std::vector<int> env_seed;
  int max_episode_steps{INT_MAX};
  int device{0};
  int env_id_offset{0};
  std::map<std::string, double> params;
  double Get(const std::string& k, double dflt) const {
    auto it = params.find(k);
    return it == params.end() ? dflt : it->second;
  }
  static Config From(const epa_config* c);
};

// Common state keys of every env (envpool/core/env_spec.h:37-43).  A family of P > 1 players gets
// "info:players.env_id", "reward" and "discount" with per-row shape [P] (one row per env, P player rows in it).
std::vector<KeySpec> CommonStateKeys(int players = 1);
constexpr int kNumCommonKeys = 8;
constexpr int kMaxKeys = 24;

// What a pool of a family produces for a config: the family's own state keys (the engine puts
// CommonStateKeys(players) in front of them), its action key, and P (a per-player key's shape starts with it).
struct FamilySpec {
  std::vector<KeySpec> state;
  KeySpec action;
  int players{1};
  std::vector<KeySpec> StateKeys() const;  // every state key of such a pool: the common ones, then `state`
};

// Output pointers handed to a step kernel: out.p[key] is the base of that
// key's [k, ...] array inside the batch block.
struct OutPtrs {
  void* p[kMaxKeys];
};

// One playout launch (Pool::Playout): k listed envs x `repeats` playouts each, entry i * repeats + r of the three
// device arrays being env row i's repeat r.
struct PlayoutArgs {
  int k;
  int repeats;
  int max_plies;            // 0: the cap
  unsigned flags;           // EPA_PLAYOUT_*
  uint64_t seed;
  float* returns;           // [k * repeats][2], 8-byte aligned
  int32_t* plies;           // [k * repeats]
  unsigned char* status;    // [k * repeats]
};

// One search launch (Pool::Search): k listed envs, row i of the three device result arrays being env row i's, and
// the tree scratch of k * (simulations + 1) nodes of the family's node size (Pool::SearchNodeBytes).
struct SearchArgs {
  int k;
  int simulations;
  int leaf_playouts;
  int max_plies;            // 0: the playouts' cap
  float c_puct;
  uint64_t seed;
  int32_t* visits;          // [k][A]
  int32_t* returns;         // [k][A]
  int32_t* action;          // [k]
  void* nodes;              // 16-byte aligned
};

// One solve launch (Pool::Solve): k listed envs, row i of the five device result arrays being env row i's, and the
// stacks of the roots' lanes, k * Pool::SolveRootBytes(depth) bytes.  table_bits > 0: the lanes' transposition tables
// behind them, k * Pool::SolveTableBytes(table_bits) bytes, all zero at the launch.
struct SolveArgs {
  int k;
  int depth;                // 0: no horizon
  long long max_nodes;
  int8_t* value;            // [k]
  int8_t* q;                // [k][A]
  int32_t* action;          // [k]
  uint8_t* status;          // [k]
  long long* nodes;         // [k], 8-byte aligned
  void* stack;              // 16-byte aligned
  void* table;              // 16-byte aligned; null without tables
  int table_bits;           // 0: no tables
};

// A device allocation whose life is shorter than its pool's: it has ONE owner, which holds it by value, and goes when
// the owner says so or dies.  (Everything that lives as long as the pool comes from Pool::DevAlloc and is freed by
// ~Pool; a buffer of one call comes from Pool::SideScratch.  This is for what a caller opens and closes: the
// guided-search session.)  Alloc and Free are called with the owner's device selected.
struct DeviceBlock {
  char* p{nullptr};
  size_t bytes{0};
  DeviceBlock() = default;
  DeviceBlock(const DeviceBlock&) = delete;
  DeviceBlock& operator=(const DeviceBlock&) = delete;
  ~DeviceBlock() { Free(); }
  void Alloc(size_t n) {
    Free();
    EPA_HIP(hipMalloc(reinterpret_cast<void**>(&p), n));
    bytes = n;
  }
  void Free() {  // (hipFree waits for the launches that still use the block)
    if (p != nullptr) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
  }
};

// One launch of a guided-search session (Pool::GuidedBegin / GuidedAdvance / GuidedResult / GuidedReroot): the
// session's k roots, its root records and nodes (family types: Pool::GuidedRootBytes / GuidedNodeBytes), and the device
// arrays the launch reads or writes -- begin, advance and reroot the three leaf arrays, advance the caller's rows,
// reroot the played actions, result its three.
struct GuidedArgs {
  int k;
  int simulations;
  int call;                 // advance: its number t = 0 .. simulations
  int capacity;             // nodes per root, the stride of a root's node block: simulations + 1 .. EPA_GUIDED_MAX_NODES
  float c_puct;
  int width;                // 0: a plain session (the plain kernels ignore it); 1 .. EPA_GUIDED_MAX_WIDTH: a wide one,
                            // whose priors, values, obs, mask and status below have k * width rows
  void* roots;              // [k], 16-byte aligned
  void* nodes;              // [k][capacity], 16-byte aligned
  const int32_t* actions;   // reroot: [k]
  const float* priors;      // [k][A]
  const float* values;      // [k]
  unsigned char* obs;       // [k][H][W][C]
  unsigned char* mask;      // [k][A]
  unsigned char* status;    // [k]
  int32_t* visits;          // [k][A]
  float* vals;              // [k][A]
  int32_t* action;          // [k]
  int flags;                // the session's EPA_GUIDED_* flags: the family chooses its kernels (last: the words above
                            // leave no padding)
};

// What opens a PUCT session (Pool::GuidedBeginCall).  The defaults are a plain session: every epa_guided_begin* entry
// point sets the fields it has and leaves the others.
struct GuidedBeginOptions {
  int simulations{0};
  int nodes{0};             // the capacity per root, simulations + 1 .. EPA_GUIDED_MAX_NODES; 0: simulations + 1
  int width{0};             // slots per root, 1 .. EPA_GUIDED_MAX_WIDTH: a wide session, whose leaf arrays have
                            // k * width rows from then on; 0: a plain session
  float c_puct{0.0f};
  int tactics{0};           // exact leaf status: the solver's horizon D, 1 .. EPA_GUIDED_MAX_TACTICS; 0: off
  long long tactics_nodes{EPA_GUIDED_TACTICS_NODES};  // ... and its node budget M per leaf
  int flags{0};             // EPA_GUIDED_PROVE: proven values
};

// One launch of a pool's recorder (Pool::RecordAdd / RecordPlan / RecordEmit; pgx_record.hip.h): the recorder's
// staging and sample arrays, all device memory of the recorder's own block, and the rows of the call.
struct RecordArgs {
  int k;                    // rows of the call
  int plies;                // staged rows per env (max_plies resolved)
  int nsym;                 // samples per staged ply: 1, or the game's symmetries
  int capacity;             // rows of the sample arrays
  int id_offset;            // env_id_offset: a sample's env_id is global
  // staging
  void* states;             // [N][plies] family positions, 16-byte aligned
  int32_t* elapsed;         // [N][plies]
  float* staged_policy;     // [N][plies][policy stride], 16-byte aligned rows
  int32_t* staged;          // [N]: n_e
  // samples
  unsigned char* obs;       // [capacity][H][W][C]
  unsigned char* mask;      // [capacity][A]
  float* policy;            // [capacity][A]
  float* value;             // [capacity]
  int32_t* ply;             // [capacity]
  int32_t* env_id;          // [capacity]
  unsigned char* sym;       // [capacity]
  int32_t* count;           // the sample count
  long long* counters;      // samples, games, dropped_games, dropped_plies
  int32_t* plan;            // [N] scratch: per row of a finish the game's first sample, or a negative code
  int32_t* items;           // [min(N plies, capacity)][2] scratch: the (row, ply) pairs a finish emits, 8-byte aligned
  int32_t* n_items;         // their number
  // the call's rows
  const float* in_policy;   // add: [k][A]
  const float* reward;      // finish: [k][2]
  const unsigned char* done;  // finish: [k]
};

// The solver stage of an advance of a guided session with tactics (Pool::GuidedTactics; pgx_guided.hip.h "Exact leaf
// status"): the horizon and the node budget of a leaf's solve, the session's counters and the slots' stacks.
struct TacticsArgs {
  int depth;                // D: 1 .. EPA_GUIDED_MAX_TACTICS
  long long max_nodes;      // M
  int32_t* decided;         // [k]: leaves decided since begin
  long long* nodes;         // [k]: positions the solver visited since begin, 8-byte aligned
  void* stack;              // [k * max(width, 1)] stacks of Pool::SolveRootBytes(D) bytes, 16-byte aligned
};

// One launch of a Gumbel-search session (Pool::GumbelBegin / GumbelAdvance / GumbelResult; pgx_gumbel.hip.h): as
// GuidedArgs, with the Gumbel noise at begin, logits instead of priors, and the improved policy among the results.
struct GumbelArgs {
  int k;
  int simulations;
  int call;                 // advance: its number t = 0 .. simulations
  int considered;           // m: the most root actions considered
  float c_visit;
  float c_scale;
  int batch;                // 0: a plain session (the plain kernels ignore it); 1 .. EPA_GUMBEL_MAX_BATCH: a batch one,
                            // whose logits, values, obs, mask and status below have k * batch rows
  void* roots;              // [k], 16-byte aligned
  void* nodes;              // [k][simulations + 1], 16-byte aligned
  const float* gumbel;      // begin: [k][A]
  const float* logits;      // [k][A]
  const float* values;      // [k]
  unsigned char* obs;       // [k][H][W][C]
  unsigned char* mask;      // [k][A]
  unsigned char* status;    // [k]
  int32_t* visits;          // [k][A]
  float* vals;              // [k][A]
  int32_t* action;          // [k]
  float* weights;           // [k][A]
};

// One step of a pool's rollout collector (Pool::RolloutStep / RolloutReset; rollout.hip.h): the rows the store kernel
// moves, the step's section of the result block, slot t of the scalar buffers, the per-env words and the episode rows.
// Every pointer is device memory.
struct RolloutStepArgs {
  rollout::StoreKeys keys;      // the obs keys (reset: into slot 0; step: into slot t + 1), then the action (slot t)
  int k;                        // rows of the batch
  int n;                        // the pool's envs
  int id_offset;                // env_id_offset: the batch's ids are global
  int capacity;                 // episode rows
  long long step;               // the collector's step counter
  const int32_t* env_id;        // the batch: [k] (null: row i is env i)
  const unsigned char* done;    // [k]
  const unsigned char* trunc;   // [k]
  const float* reward;          // [k]
  float* rew;                   // slot t: [N]
  unsigned char* term;
  unsigned char* trc;
  unsigned char* mask;
  unsigned char* carry;         // per env: [N]
  double* acc_ret;
  int32_t* acc_len;
  unsigned char* emit;          // this step's emission flags, 16-byte aligned, and what is emitted
  double* emit_ret;
  int32_t* emit_len;
  int32_t* ep_env;              // episodes: [capacity]
  long long* ep_step;
  double* ep_ret;
  int32_t* ep_len;
  rollout::Control* ctl;
};
// The collector's kernels (rollout.hip), one launch each on `s`
void RolloutLaunchStore(const RolloutStepArgs& a, bool scalars, hipStream_t s);
void RolloutLaunchScan(const RolloutStepArgs& a, hipStream_t s);
void RolloutLaunchGae(int horizon, int n, const float* reward, const unsigned char* term, const unsigned char* trunc,
                      const unsigned char* mask, const float* values, float gamma, float lam, float* adv, float* ret,
                      hipStream_t s);
// x: [n][comps] of EPA_F32 / EPA_F64 -> partial [groups][comps_total][2] at component comp0; then the fold into acc
// (count, sum, sumsq: [3][comps_total])
void RolloutLaunchMoments(const void* x, int dtype, int n, int comps, int comp0, int comps_total, double* partial,
                          hipStream_t s);
void RolloutLaunchMomentsFold(const double* partial, int n, int comps_total, double* acc, hipStream_t s);

struct Batch {
  // where the batch's kernels write and recv reads: the block's own device allocation (`dev_buf`), or -- a DIRECT
  // step, Pool::SendInto -- the caller's pinned host block, where the results then already are when recv wants them
  char* dbuf{nullptr};
  char* dev_buf{nullptr};
  bool direct{false};
  size_t cap_rows{0};
  int k{0};
  int consumed{0};                // rows already handed to recv (async mode)
  std::vector<size_t> offsets;    // byte offset of each key's section
  hipEvent_t done{nullptr};
  // single-stream pools record `done` only when somebody needs it (Pool::EnsureDone): an event record behind
  // every launch keeps consecutive step kernels further apart than the launch path alone
  bool done_recorded{false};
  // A whole-pool host-path step of a sync pool may be cut into TWO launches (Pool::Send, "step_pipeline"): rows
  // [0, part_rows) are complete at `part_ev`, so their download overlaps the second launch
  int part_rows{0};               // 0: one launch
  hipEvent_t part_ev{nullptr};
  hipStream_t stream{nullptr};    // the compute stream its kernel was launched on ...
  int stream_idx{0};              // ... and always will be: blocks are recycled per stream
  // async mode with several compute streams: the local env of every row (host-path sends / resets;
  // empty for device-path batches, whose ids the host never sees), so that recv can mark them idle
  std::vector<int32_t> host_ids;
};

// Per-env bookkeeping shared by all families, SoA on device:
//   cur_step  Env::current_step_ (env.h:86)      init -1
//   done      XxxEnv::done_                       init 1 (first step resets)
//   mt/mti    std::mt19937 gen_ (env.h:78)        624 words per env + the position of the next word.
//             Layout: mt_shift = 0 the plain [624][N] structure of arrays, mt_shift = 4 tiles of 16 consecutive
//             words of one env, tile t of all envs = one [N][16] slab (device_common.hip.h: Mt19937::At)
struct CommonDev {
  int* cur_step;
  unsigned char* done;
  uint32_t* mt;
  int* mti;
  int n;
  int mt_shift;
};

// A few helper threads that copy one big host buffer into the pinned staging slot in pieces, together with the
// calling thread: a 3 MB action batch takes one thread 0.12 ms (25 GB/s), and in the sync step() that copy is in front
// of everything else (the reference hands its workers POINTERS into the caller's array, py_envpool.h:89-101; a
// device cannot read pageable memory).  Pieces are claimed with an atomic counter; the caller watches the in-order
// frontier of finished pieces and uploads behind it.  Workers poll for ~0.3 ms after a job (the next step's send
// is that close in a step loop) and sleep on a condition variable otherwise.
// CPUs of the NUMA node of `device` (empty if unknown), engine.hip
std::vector<int> DeviceLocalCpus(int device);

class HostCopier {
 public:
  static constexpr size_t kPiece = 256u << 10;
  // `cpus`: where the helpers may run (the device's NUMA node, DeviceLocalCpus; empty = anywhere)
  HostCopier(int threads, const std::vector<int>& cpus);
  ~HostCopier();
  HostCopier(const HostCopier&) = delete;
  HostCopier& operator=(const HostCopier&) = delete;
  void Start(char* dst, const char* src, size_t bytes);
  // The caller copies pieces too until bytes [0, upto) are in place; returns the bytes in place (a multiple of
  // kPiece, or the total), which may be more.
  size_t Advance(size_t upto);

 private:
  // One copy job; immutable but for the claim counter and the per-piece flags.  A helper that is late for a job finds
  // every piece claimed and leaves it alone: the next job never has to wait for stragglers.
  struct Job {
    char* dst;
    const char* src;
    size_t bytes, pieces;
    std::atomic<size_t> next{0};
    std::unique_ptr<std::atomic<uint8_t>[]> done;
  };
  void Work();
  static bool CopyOne(Job& j);
  std::vector<std::thread> th_;
  std::mutex mu_;
  std::condition_variable cv_;
  std::atomic<uint64_t> gen_{0};
  std::atomic<bool> stop_{false};
  std::shared_ptr<Job> job_;   // guarded by mu_
  std::shared_ptr<Job> mine_;  // the caller's handle on the current job
  size_t frontier_{0};         // pieces [0, frontier_) are complete (the caller's view)
};

// The PGX built-in network (pgx_net.hip.h is the contract, pgx_net.hip the kernel).  NetImage is a checked blob in the
// kernel's layout: per layer the weights in 1 KiB (output tile, k-step) blocks and the bias padded to whole tiles.
constexpr int kNetImageLayers = 18;  // 2 * 8 blocks + trunk + head
struct NetImage {
  int F{0}, A{0}, D{0}, L{0}, layers{0};
  float scale_p{0}, scale_v{0};
  std::vector<char> bytes;
  uint32_t w_off[kNetImageLayers]{}, b_off[kNetImageLayers]{};
  int32_t shift[kNetImageLayers]{};
};
// std::invalid_argument with NetParse's reason for a blob that is no network
void NetBuildImage(const void* blob, size_t bytes, NetImage* out);
// One PgxNetEval on `stream`: obs u8 [rows][F], mask u8 [rows][A], status u8 [rows] -> policy f32 [rows][A], value f32
// [rows]; mode: kNetLogits 0 / kNetPriors 1; pending (or null): ORed with 1 when some row's status is not 2.
void NetLaunch(const NetImage& im, const char* d_image, int rows, int mode, const unsigned char* obs,
               const unsigned char* mask, const unsigned char* status, float* policy, float* value,
               unsigned int* pending, hipStream_t stream);
// The rollout actor's form (actor.hip.h): features u8 [rows][F] with bytes 0 .. 127, every row evaluated -> the head's
// int32 p [rows][A + 1], nothing else
void NetLaunchRaw(const NetImage& im, const char* d_image, int rows, const unsigned char* features, int32_t* head,
                  hipStream_t stream);
// The rollout actor's own kernels (actor.hip; actor.hip.h is the contract), one launch each on `s`.  Every pointer is
// device memory.
namespace actor {
struct FeatureKeys;
}
struct ActorSampleArgs {
  int rows;                     // row i: env id_offset + i, or env_id[i]
  int H, kind;                  // actor::kDiscrete / kBox
  int deterministic;
  int value_only;               // only value [rows] is written
  int id_offset;
  const int32_t* env_id;        // global ids [rows], or null
  long long step;               // the collector's step counter: the noise's
  uint64_t seed;
  float scale_p, scale_v;
  const float* sigma;           // box: [H] each
  const float* low;
  const float* high;
  const int32_t* head;          // [rows][H + 1]
  void* action;                 // int32 [rows], or the action dtype's [rows][H]
  int action_dtype;
  float* logp;                  // [rows]
  float* value;                 // [rows]
};
// obs rows -> features u8 [rows][F], 16-byte stores where the output allows
void ActorLaunchFeatures(const actor::FeatureKeys& keys, const double* lo, const double* scale, int rows,
                         unsigned char* out, hipStream_t s);
void ActorLaunchSample(const ActorSampleArgs& a, hipStream_t s);
// The pair form (pgx_arena.hip.h).  NetPlanLaunch: PgxNetPlan, the stable partition of `rows` <= 2^20 rows by `side` u8
// [rows] into order i32 [rows] and n0 i32 [1], with `counts` (NetPlanCountBytes(rows) bytes) as its scratch.
// NetLaunchPair: one pair PgxNetEval, row r by net side[r] through that plan; both nets of one F and A.
constexpr int kNetPlanMaxRows = 1 << 20;  // pgx::kArenaMaxRows
size_t NetPlanCountBytes(size_t rows);
void NetPlanLaunch(int rows, const unsigned char* side, int32_t* counts, int32_t* order, int32_t* n0,
                   hipStream_t stream);
void NetLaunchPair(const NetImage& im_a, const char* d_image_a, const NetImage& im_b, const char* d_image_b, int rows,
                   int mode, const int32_t* order, const int32_t* n0, const unsigned char* obs,
                   const unsigned char* mask, const unsigned char* status, float* policy, float* value,
                   unsigned int* pending, hipStream_t stream);

// A network on a device (epa_net_create): it belongs to the device, not to a pool, and owns ONE device allocation --
// the image, the pending word, the policy / value rows its evaluations inside epa_net_run and the host forms write,
// and the plan (order, counts, n0) of the pair evaluations it leads as net A, grown to the largest `rows` seen.  Calls on one net are the caller's to serialise, as a pool's session is.
class Net {
 public:
  Net(int device, const void* blob, size_t bytes);
  int device() const { return device_; }
  const NetImage& image() const { return image_; }
  void Reserve(size_t rows);  // (growing waits for the launches that use the old block)
  const char* d_image() const { return mem_.p; }
  unsigned int* pending() const { return reinterpret_cast<unsigned int*>(mem_.p + image_.bytes.size()); }
  float* value() const { return reinterpret_cast<float*>(mem_.p + image_.bytes.size() + 256); }
  float* policy() const { return value() + rows_; }  // (rows_ is a multiple of 64)
  int32_t* plan_n0() const { return reinterpret_cast<int32_t*>(mem_.p + image_.bytes.size() + 64); }
  int32_t* plan_order() const { return reinterpret_cast<int32_t*>(policy() + rows_ * (size_t)image_.A); }
  int32_t* plan_counts() const { return plan_order() + rows_; }

 private:
  int device_;
  NetImage image_;
  DeviceBlock mem_;
  size_t rows_{0};
};

// One launch of a pool's self-play driver (Pool::SelfplayNoise / SelfplayMove / SelfplayTally; pgx_selfplay.hip.h):
// row i is local env i of the pool, every pointer device memory.
struct SelfplayArgs {
  int k;                        // rows: the pool's envs
  int id_offset;                // env_id_offset: a key takes the global id
  int policy;                   // EPA_SELFPLAY_GUMBEL / EPA_SELFPLAY_PUCT
  int noise;                    // 0: zero rows
  int sample_plies;
  uint32_t t;                   // the ply counter
  uint64_t seed;
  float* gumbel;                // noise: [k][A] out
  const int32_t* visits;        // move, PUCT: the result's [k][A]
  const int32_t* result_action; // move: the result's [k]
  const int32_t* cur_step;      // move, PUCT: the envs' elapsed steps [N] (the family hook fills it in)
  const float* weights;         // move, Gumbel: the result's [k][A]
  int32_t* action;              // move: [k] out, the step's action row
  float* target;                // move: [k][A] out, the recorder's policy rows
  const unsigned char* done;    // tally: the step's result block
  const float* reward;          // [k][2]
  const int32_t* elapsed;       // [k]
  long long* counters;          // tally: [5] (an arena: [7]), 8-byte aligned
  int arena;                    // tally: 0 / 1, the seven counters of pgx_arena.hip.h
  int slots;                    // arena sides: leaf rows per env
  unsigned char* side;          // arena sides: [k * slots] out
  // PUCT exploration (pgx_dirichlet.hip.h)
  float alpha, gamma_d, gamma_c;  // dirichlet: alpha and the host-rounded d and c of its sampler
  float eps;                      // dirichlet: the mix
  float temperature;              // move, PUCT: 1 is the plain rule
  const unsigned char* mask;      // dirichlet: the leaf rows' legal actions [k * slots][A]
  const unsigned char* status;    // dirichlet: the leaf rows' status [k * slots]
  float* prior;                   // dirichlet: the evaluator's policy rows [k * slots][A], mixed in place
};

// What a driver is opened with (include/envpool_amd.h: epa_selfplay_options)
using SelfplayOptions = epa_selfplay_options;
using SelfplayExtra = epa_selfplay_extra;  // (epa_selfplay_begin_ex; {0, 0, 1, 0} is the plain driver)
// The driver's kernels (pgx_selfplay.hip) for PGX game `game` (pgx::kTicTacToe ...), one launch each on `stream`
void PgxSelfplayLaunchNoise(int game, const SelfplayArgs& a, hipStream_t stream);
void PgxSelfplayLaunchMove(int game, const SelfplayArgs& a, hipStream_t stream);
void PgxSelfplayLaunchTally(const SelfplayArgs& a, hipStream_t stream);  // (a.arena: PgxArenaTally)
void PgxSelfplayLaunchDirichlet(int game, const SelfplayArgs& a, hipStream_t stream);

class Pool {
 public:
  // `spec`: the family's describe result for cfg; the state keys become CommonStateKeys(spec.players) + spec.state
  Pool(const Config& cfg, const FamilySpec& spec, bool needs_rng);
  virtual ~Pool();

  const Config& cfg() const { return cfg_; }
  const std::vector<KeySpec>& state_keys() const { return keys_; }
  const KeySpec& action_key() const { return action_; }
  hipStream_t stream() const { return stream_; }

  // The host-facing entry points are virtual: a family whose env bodies run on the HOST
  // (Atari: ALE stays on the CPU, north star) replaces the stream-ordered execution with
  // its own executor and keeps the C ABI (atari_env.hip).
  virtual void Send(const int32_t* env_id, int k, const void* action);
  // Send whose results may land straight in `block` (see epa_send_into); families with their own executor ignore the block
  virtual void SendInto(const int32_t* env_id, int k, const void* action, void* block, size_t block_bytes);
  virtual void Reset(const int32_t* env_ids, int k);
  virtual void SendDevice(const int32_t* d_env_id, int k, const void* d_action,
                          hipEvent_t wait_event = nullptr);
  // stream_ waits for everything enqueued so far on `producer` (device path)
  void WaitStream(hipStream_t producer);
  // `consumer` waits for the kernel of the batch RecvDevice handed out last
  void ConsumerWait(hipStream_t consumer);
  virtual int Recv(void* const* out_ptrs, int n_ptrs, int cap_rows);
  // zero-copy host recv into a caller-owned block (see epa_recv_block)
  size_t RecvLayout(int rows, size_t* offsets, int n_keys) const;
  virtual int RecvBlock(void* block, size_t block_bytes, size_t* offsets, int n_keys);
  virtual int RecvInto(void* const* out_ptrs, int n_ptrs, int cap_rows);
  virtual int RecvDevice(void** d_out_ptrs, int n_ptrs);
  virtual int PendingRows();
  virtual void Synchronize();
  void SetTiming(int mode);  // 0 off, 1 an event pair around every launch, 2 one pair around the whole window
  void KernelTime(double* avg_ms, int* launches);

  // May launches of this family run concurrently on several streams (async mode)?  True only if
  // a launch touches nothing but the per-env state of ITS rows and its own result block: no
  // per-launch scratch shared through the pool (the Humanoid kernels' HBM workspace and sort
  // buffer are indexed by the wave of the launch: they say no and keep one compute stream).
  virtual bool ConcurrentSafe() const { return false; }
  virtual int StateDim() const = 0;
  // family hooks: flat double state <-> device SoA, for the listed local ids
  virtual void GetState(const int* d_ids, int k, double* d_out) = 0;
  virtual void SetState(const int* d_ids, int k, const double* d_in) = 0;
  void GetStateHost(const int32_t* ids, int k, double* out);
  void SetStateHost(const int32_t* ids, int k, const double* in);
  // render (rgb_array mode; RenderableEnv of envpool/core/env.h, AsyncEnvPool::Render): RenderSize resolves a
  // width / height <= 0 to the env's default, Render paints uint8 [k, h, w, 3] frames of the listed local envs
  // from their persistent state on stream_ (d_rgb: any alignment).  A family that does not render keeps the
  // defaults, which throw the reference's std::runtime_error("render not implemented for this environment").
  virtual void RenderSize(int width, int height, int* w, int* h) const;
  virtual void Render(const int* d_ids, int k, int w, int h, int camera_id, void* d_rgb);
  // The host entry points (epa_render_size / epa_render / epa_render_device).  A frame shows its env after every
  // send issued before the call, received or not.  RenderHost returns the frames in host memory; RenderDevice
  // only enqueues (no host copy, no host wait): the frames are complete once the pool's stream has passed.
  void RenderSizeHost(int width, int height, int* w, int* h) const;
  void RenderHost(const int32_t* ids, int k, int width, int height, int camera_id, uint8_t* out);
  void RenderDevice(const int32_t* ids, int k, int width, int height, int camera_id, void* d_out);

  // Snapshots (snapshot.hip.h: blob layout and kernels): everything that makes the listed envs continue bit for bit --
  // the flat state, with EPA_SNAP_RNG the generator words and their position, the observation ring of frame_stack > 1
  // and the family's extra section -- as one opaque blob, written and read on stream_.  A snapshot shows each env after
  // every send issued before the call, received or not; a restore takes effect before every send issued after it and
  // leaves rows already in the result queue alone.  Restore and fork targets must not repeat.  A family without a flat
  // state (StateDim() == 0) throws std::runtime_error("snapshot not implemented for this environment") from all of
  // them.  The *Device forms only enqueue (the blob is device memory, 16-byte aligned); *Host copy the blob across
  // once.  Fork: env dst[i] becomes env src[i] (src may repeat and overlap dst: it is a snapshot followed by a restore).
  void SetFamily(const std::string& name);  // what the blob's family hash is taken from (epa_create)
  size_t SnapshotBytes(int k, unsigned flags) const;
  // host_header (optional): receives the blob's 64-byte header, which RestoreDevice wants back from the host
  void SnapshotDevice(const int32_t* ids, int k, unsigned flags, void* d_blob, void* host_header = nullptr);
  void RestoreDevice(const int32_t* ids, int k, const void* d_blob, const void* host_header);
  void SnapshotHost(const int32_t* ids, int k, unsigned flags, void* out, size_t out_bytes);
  void RestoreHost(const int32_t* ids, int k, const void* blob, size_t blob_bytes);
  void Fork(const int32_t* src, const int32_t* dst, int k, unsigned flags);

  // Random playouts (include/envpool_amd.h: epa_playout; the PGX board games, pgx_playout.hip.h): every listed env is
  // played on `repeats` times from the state every send issued before the call has left it in, to the end of its game
  // or for max_plies plies, with uniformly drawn legal actions; what comes back is the per-player return, the plies
  // played and a status per playout.  Nothing of the pool changes -- unless EPA_PLAYOUT_COMMIT asks for the final
  // states to be written back, which then takes effect before every send issued after the call, like a restore.
  // The family hook launches on stream_ for local ids; a family without one keeps the defaults, and both entry points
  // throw std::runtime_error("playout not implemented for this environment").  PlayoutHost returns the results in host
  // memory (one stream synchronisation); PlayoutDevice only enqueues.
  virtual bool HasPlayout() const { return false; }
  virtual void Playout(const int* d_ids, const PlayoutArgs& a);
  void PlayoutHost(const int32_t* ids, int k, int repeats, int max_plies, uint64_t seed, unsigned flags, float* returns,
                   int32_t* plies, uint8_t* status);
  void PlayoutDevice(const int32_t* ids, int k, int repeats, int max_plies, uint64_t seed, unsigned flags,
                     void* d_returns, void* d_plies, void* d_status);

  // Tree search (include/envpool_amd.h: epa_search; the PGX board games, pgx_search.hip.h): for every listed env,
  // `simulations` rounds of PUCT selection from the state every send issued before the call has left it in, with
  // uniform priors and `leaf_playouts` random playouts per new leaf; what comes back is the root's visit counts and
  // summed returns per action and the most visited action.  Nothing of the pool changes.  The family hook launches on
  // stream_ for local ids, its tree in `a.nodes` (the side scratch block); a family without one keeps the defaults,
  // and both entry points throw std::runtime_error("search not implemented for this environment").  SearchHost returns
  // the results in host memory (one stream synchronisation); SearchDevice only enqueues.
  virtual bool HasSearch() const { return false; }
  virtual int SearchActions() const { return 0; }        // A: the width of a result row
  virtual size_t SearchNodeBytes() const { return 0; }   // a multiple of 16
  virtual void Search(const int* d_ids, const SearchArgs& a);
  void SearchHost(const int32_t* ids, int k, int simulations, int leaf_playouts, float c_puct, int max_plies,
                  uint64_t seed, int32_t* visits, int32_t* returns, int32_t* action);
  void SearchDevice(const int32_t* ids, int k, int simulations, int leaf_playouts, float c_puct, int max_plies,
                    uint64_t seed, void* d_visits, void* d_returns, void* d_action);

  // Exact solve (include/envpool_amd.h: epa_solve; the PGX board games, pgx_solve.hip.h): for every listed env, the
  // minimax value of its position -- to the end of the game, or to a horizon of `depth` plies -- per root action, by
  // alpha-beta in one launch.  Nothing of the pool changes.  The family hook launches on stream_ for local ids, the
  // lanes' stacks in `a.stack` (the side scratch block); a family without one keeps the defaults, and both entry
  // points throw std::runtime_error("solve not implemented for this environment").  A row is SearchActions() wide.
  // SolveHost returns the results in host memory (one stream synchronisation); SolveDevice only enqueues.
  virtual bool HasSolve() const { return false; }
  virtual size_t SolveRootBytes(int /*depth*/) const { return 0; }  // a root's stacks; a multiple of 16
  virtual size_t SolveTableBytes(int /*table_bits*/) const { return 0; }  // a root's tables; a multiple of 16
  virtual void Solve(const int* d_ids, const SolveArgs& a);
  // table_bits = b > 0 (epa_solve_table): every lane's private transposition table of 2^b entries, behind the stacks
  // in the side scratch block, cleared on stream_ before the launch; 0: no tables, and no further launch.
  void SolveHost(const int32_t* ids, int k, int depth, long long max_nodes, int table_bits, int8_t* value, int8_t* q,
                 int32_t* action, uint8_t* status, int64_t* nodes);
  void SolveDevice(const int32_t* ids, int k, int depth, long long max_nodes, int table_bits, void* d_value, void* d_q,
                   void* d_action, void* d_status, void* d_nodes);

  // Guided tree search (include/envpool_amd.h: epa_guided_begin; the PGX board games, pgx_guided.hip.h): a search
  // whose tree stays on the device between launches and that stops at every new leaf, so that the caller supplies
  // the priors and the leaf values.  A pool has at most one session.  Its memory -- root records, nodes and the
  // staging of the host forms -- is ONE device allocation of its own (not the side scratch block, which search, render
  // and snapshot reuse between two advances), released by GuidedEnd, by the next begin and by ~Pool.  Every call
  // enters through SideEnter like the other side operations: begin sees the state every send issued before it has
  // left, and the session's launches are ordered behind each other on whichever stream they land.  The host forms
  // copy through the session's pinned block and synchronise once; the device forms only enqueue and leave through
  // SideLeave: SessionRun below is that path, for every call of either policy.  A family without the hooks keeps the defaults, and every entry point throws
  // std::runtime_error("guided search not implemented for this environment").
  virtual bool HasGuided() const { return false; }
  virtual void GuidedShape(int32_t shape[4]) const { shape[0] = shape[1] = shape[2] = shape[3] = 0; }  // H, W, C, A
  virtual size_t GuidedNodeBytes() const { return 0; }   // multiples of 16
  virtual size_t GuidedRootBytes() const { return 0; }
  virtual void GuidedBegin(const int* d_ids, const GuidedArgs& a);
  virtual void GuidedAdvance(const GuidedArgs& a);
  virtual void GuidedResult(const GuidedArgs& a);
  virtual void GuidedReroot(const GuidedArgs& a);
  // exact leaf status (pgx_guided.hip.h "Exact leaf status"): the solver stage after an advance's descents
  virtual void GuidedTactics(const GuidedArgs& a, const TacticsArgs& t);
  // proven values (pgx_guided.hip.h "Proven values"): the read-out of a session begun with EPA_GUIDED_PROVE (value
  // int8 [k], q int8 [k][A], device memory)
  virtual void GuidedProof(const GuidedArgs& a, signed char* value, signed char* q);
  // wide sessions (pgx_guided.hip.h "Several leaves per launch", a.width slots per root) and sessions with proven
  // values (a.flags) go through the hooks above too: the family chooses its kernels by a.width and a.flags
  virtual size_t GuidedWideRootBytes(int width) const { (void)width; return 0; }  // a multiple of 16
  virtual size_t GuidedWideLiveOffset() const { return 0; }  // of a record's int32 count of pending slots
  // The one begin of a PUCT session, whatever its options.  obs / mask / status: host arrays (device == false) or
  // device pointers.  check_only: the call's refusals and nothing else (the self-play driver's begin asks them before
  // its first ply).
  void GuidedBeginCall(const int32_t* ids, int k, const GuidedBeginOptions& o, void* obs, void* mask, void* status,
                       bool device, bool check_only = false);
  // Exact leaf status: the session's counters, decided int32 [k] and (may be null) the solver's visited positions
  // int64 [k]; zeros for a session without tactics; the device form only enqueues.
  void GuidedDecidedCall(void* decided, void* nodes, bool device);
  // Proven values: value int8 [k] and q int8 [k][A]; -128 everywhere for a session without EPA_GUIDED_PROVE; the
  // device form only enqueues.
  void GuidedProofCall(void* value, void* q, bool device);
  // Tree reuse (pgx_guided.hip.h "Tree reuse"): after the round's last advance, the subtree under actions[i] becomes
  // root i's tree, `simulations` the length of the next round, and the new roots are emitted as begin emits its own.
  // actions: a host array (checked against 0 .. A-1 here) or a device pointer (the kernel ends such a root).  PUCT
  // sessions only.
  void GuidedRerootCall(const void* actions, int k, int simulations, void* obs, void* mask, void* status, bool device);
  void GuidedAdvanceCall(const void* priors, const void* values, int k, void* obs, void* mask, void* status,
                         bool device);
  void GuidedResultCall(void* visits, void* values, void* action, bool device);
  void GuidedEnd();

  // Gumbel search (include/envpool_amd.h: epa_gumbel_begin; pgx_gumbel.hip.h): the guided-search session with a
  // second selection policy.  It IS the pool's guided-search session -- the same single-owner allocation, released by
  // GuidedEnd, by the next begin of either policy and by ~Pool -- and enters through the side-operation path as the
  // Guided calls do.  The other policy's advance and result refuse an open session with std::invalid_argument.  A
  // family that has guided search has Gumbel search; the others throw
  // std::runtime_error("gumbel search not implemented for this environment").
  virtual size_t GumbelNodeBytes() const { return 0; }   // multiples of 16
  virtual size_t GumbelRootBytes() const { return 0; }
  virtual void GumbelBegin(const int* d_ids, const GumbelArgs& a);
  virtual void GumbelAdvance(const GumbelArgs& a);
  virtual void GumbelResult(const GumbelArgs& a);
  // batch sessions (pgx_gumbel.hip.h "A level per launch"): a.batch slots per root; the three hooks above serve them
  // too (a.batch != 0: the family chooses its kernels)
  virtual size_t GumbelBatchRootBytes(int batch) const { (void)batch; return 0; }  // a multiple of 16
  // The one begin of a Gumbel session.  batch: slots per root, 1 .. EPA_GUMBEL_MAX_BATCH: the leaf arrays have
  // k * batch rows from then on (the noise keeps k); 0: a plain session.
  // check_only: as GuidedBeginCall's.
  void GumbelBeginCall(const int32_t* ids, int k, int simulations, int considered, int batch, float c_visit,
                       float c_scale, const void* gumbel, void* obs, void* mask, void* status, bool device,
                       bool check_only = false);
  void GumbelAdvanceCall(const void* logits, const void* values, int k, void* obs, void* mask, void* status,
                         bool device);
  void GumbelResultCall(void* visits, void* values, void* action, void* weights, bool device);

  // The built-in network (include/envpool_amd.h: epa_net_eval, epa_net_run).  Both refuse a family without guided
  // search as the guided calls do, and a net of another device or of another F / A than GuidedShape's with
  // std::invalid_argument.  NetEvalCall: one evaluation of `rows` caller rows, enqueued on stream_ (host form: staged
  // through the side scratch, complete on return).  NetRunCall: `advances` pairs of (PgxNetEval, the open session's
  // advance through Guided / GumbelAdvanceCall's device path) on the leaf arrays, which are in / out; 0: until the
  // round is complete -- a plain session: simulations + 1 - calls pairs without a host wait; a wide or batch session:
  // one read of the pending word per pair.  Returns the pairs made.
  void NetEvalCall(Net& net, int rows, int mode, const void* obs, const void* mask, const void* status, void* policy,
                   void* value, bool device);
  // `after_first` (the self-play driver's Dirichlet mix): called once, with the lock held and the side operation
  // entered, behind the call's first evaluation and before its first advance, with the policy rows it may change.
  using NetRunHook = std::function<void(float* policy)>;
  int NetRunCall(Net& net, int advances, void* obs, void* mask, void* status, bool device,
                 const NetRunHook* after_first = nullptr);
  // The pair forms (pgx_arena.hip.h): row r is evaluated by net_a where side[r] == 0 and by net_b where it is 1; both
  // nets pass NetRequire and so agree in F and A.  NetEvalPairCall: PgxNetPlan + one pair PgxNetEval of `rows` <= 2^20
  // caller rows with the caller's side bytes (host form: a byte other than 0 / 1 is refused; staged like
  // NetEvalCall's).  NetRunPairCall: NetRunCall's device form with `side` u8 device memory, one byte per leaf row,
  // fixed for the call: the plan is made once, and policy / value rows and the plan live in net_a's allocation.
  void NetEvalPairCall(Net& net_a, Net& net_b, int rows, int mode, const void* obs, const void* mask,
                       const void* status, const void* side, void* policy, void* value, bool device);
  int NetRunPairCall(Net& net_a, Net& net_b, int advances, void* obs, void* mask, void* status, const void* side,
                     const NetRunHook* after_first = nullptr);

  // Self-play recorder (include/envpool_amd.h: epa_record_begin; the PGX board games, pgx_record.hip.h): stages every
  // env's positions and policy targets while its game runs and turns a finished game into training samples in a
  // sample buffer on the device.  A pool has at most one recorder.  Its memory -- staging, samples, counters, the
  // rows of the host forms -- is ONE device allocation of its own with a single owner, released by RecordEnd, by the
  // next RecordBegin and by ~Pool; it is independent of the guided session's, and the two coexist.  Every call enters
  // through SideEnter, so add sees the state every send issued before it has left.  The host forms copy the call's rows
  // through the recorder's pinned block and synchronise once (drain: once for the count, once for the rows); the device
  // forms only enqueue and leave through SideLeave.  A family without the hooks keeps the defaults, and every entry
  // point throws std::runtime_error("recorder not implemented for this environment").
  virtual bool HasRecord() const { return false; }
  virtual int RecordSyms() const { return 1; }            // the game's symmetries (EPA_RECORD_SYMMETRIES)
  virtual size_t RecordStateBytes() const { return 0; }   // a staged position; a multiple of 16
  virtual int RecordPolicyStride() const { return 0; }    // floats of a staged policy row; a multiple of 4
  virtual void RecordAdd(const int* d_ids, const RecordArgs& a);
  virtual void RecordPlan(const int* d_ids, const RecordArgs& a);
  virtual void RecordEmit(const int* d_ids, const RecordArgs& a);
  void RecordBegin(int capacity, int max_plies, unsigned flags);
  // policy [k][A] float32; host ids must not repeat (refused); device == true: `policy` is device memory
  void RecordAddCall(const int32_t* ids, int k, const void* policy, bool device);
  // reward [k][2] float32 and done [k] bytes: what the step returned
  void RecordFinishCall(const int32_t* ids, int k, const void* reward, const void* done, bool device);
  // the first `rows` samples into seven host arrays (rows must equal the sample count, which *count receives in any
  // case; a mismatch throws and leaves the recorder as it is), then the count is 0
  void RecordDrain(int rows, void* const out[7], int32_t* count);
  void RecordView(void* out[7], void** count) const;  // the seven device arrays over the capacity, the device count
  void RecordClear();                                  // count = 0; only enqueues
  void RecordDiscard(const int32_t* ids, int k);       // n_e = 0 for the listed envs
  void RecordCounters(int64_t out[5]);                 // count, samples, games, dropped_games, dropped_plies
  void RecordShape(int32_t out[5]) const;              // H, W, C, A, nsym of the open recorder
  void RecordEnd();

  // Rollout collector (include/envpool_amd.h: epa_rollout_begin; rollout.hip.h is the contract): an on-policy
  // trajectory buffer in device memory that the pool's own step fills -- RolloutStep is SendDevice + the collector's
  // kernels on the batch's stream + Recv / RecvDevice, so the rows are read from the result block in HBM.  It belongs to
  // the base pool: every family with one row per env and a device step has it (HasRollout; PGX, two rows per env, and
  // the host-stepped Atari pool throw std::runtime_error("rollout not implemented for this environment")).  A pool
  // in sync mode only.  A pool has at most one collector; its memory is ONE device allocation of its own with a single
  // owner, released by RolloutEnd, by the next RolloutBegin and by ~Pool.  While one is open, Reset is refused
  // (std::invalid_argument): an env reset behind the collector's back would break its mask and episode accounting.
  // The device forms only enqueue; the host forms end in one stream synchronisation.  Calls on one collector are the
  // caller's to serialise.
  virtual bool HasRollout() const;
  void RolloutBegin(int horizon, int episodes, unsigned flags);
  void RolloutShape(int64_t out[8]) const;  // T, N, episodes, t, obs keys, moment components, step counter, flags
  int RolloutReset(bool device, void** ptrs, int n_ptrs, int cap_rows);
  int RolloutStep(bool device, const void* action, hipEvent_t wait_event, void** ptrs, int n_ptrs, int cap_rows);
  // the device arrays: one per obs key, then action, reward, term, trunc, mask
  void RolloutView(void** arrays, int n) const;
  void RolloutBatch(void* const* out, int n);  // the same arrays, whole, copied to the host
  void RolloutGae(bool device, const void* values, float gamma, float lam, void* adv, void* ret);
  void RolloutEpisodes(int rows, int32_t* env_id, int64_t* step, double* ret, int32_t* length, int32_t* count);
  void RolloutEpisodesView(void* out[4], void** count) const;
  void RolloutMoments(double* host_out, void** d_out);  // [3][components]: count, sum, sumsq
  void RolloutNext();
  void RolloutCounters(int64_t out[6]);  // count, finished, dropped, step counter, t, started
  void RolloutEnd();

  // Rollout actor (include/envpool_amd.h: epa_actor_begin; actor.hip.h is the contract): a built-in actor-critic
  // attached to the open collector, so that RolloutCollect plays whole steps from C++ -- features of slot t, the int8
  // trunk (PgxNetEval's raw form), the sample, then exactly what RolloutStep enqueues -- with no host wait in between.
  // ActorBegin checks the blob (ActorParse) and compares it with the pool: F = the obs keys' components, the action
  // dtype and row with the blob's kind and H, `actions` (the caller's count of discrete actions, or the Box dimension)
  // with H; a mismatch, or a pool without an open collector, is std::invalid_argument.  low / high: the Box bounds,
  // [H] each (ignored for a discrete space).  Its memory -- the net image, lo / scale, sigma and the bounds, the
  // feature rows, the head's rows, logp [T][N] and value [T+1][N] -- is ONE device allocation of its own, counted with
  // the collector's in the 2 GiB limit, released by ActorEnd, by the next ActorBegin and with the collector.
  // RolloutCollect: `steps` steps (0: the rest of the horizon), then the value of slot t; device: only enqueues,
  // otherwise ONE stream synchronisation at the end.  With an actor attached RolloutGae takes values == nullptr for
  // the stored ones.  ActorEval, a side operation: (action, logp, value) of k rows of caller observations (one array
  // per obs key) for the listed global env ids at step counter `step`; nothing of the pool changes.
  void ActorBegin(const void* blob, size_t bytes, uint64_t seed, unsigned flags, int actions, const double* low,
                  const double* high);
  void ActorEnd();
  void ActorShape(int64_t out[4]);  // F, H, kind, flags of the attached actor
  void ActorEval(bool device, const int32_t* ids, int k, long long step, const void* const* obs, int n_obs,
                 void* action, void* logp, void* value);
  void ActorView(void** logp, void** value);  // the device arrays [T][N] and [T+1][N]
  void ActorBatch(float* logp, float* value);       // the same, whole, copied to the host
  void RolloutCollect(int steps, bool device);

  // Self-play driver (include/envpool_amd.h: epa_selfplay_begin; the PGX board games, pgx_selfplay.hip.h): plays
  // plies of every env of the pool with a Net as the evaluator, through the device forms of the calls above --
  // GumbelBeginCall / GuidedBeginCall, NetRunCall, *ResultCall, RecordAddCall, SendDevice, RecvDevice, RecordFinishCall --
  // and three launches of its own in between (four with Dirichlet root noise).  A pool has at most one driver.  Its memory -- noise, leaf arrays, result
  // arrays, action row, target rows, counters -- is ONE device allocation of its own with a single owner, released by
  // SelfplayEnd, by the next SelfplayBegin and by ~Pool; it coexists with the session (which the driver opens ply by
  // ply, and whose last one stays open) and the recorder.  SelfplayRun only enqueues (device == false: then waits for
  // the stream); SelfplayStats is the one host wait.  The net must outlive the driver.  A SelfplayRun that throws
  // partway has enqueued its earlier plies and part of one more (a recorder add without its finish) and does not
  // count the partial ply in t: the driver must be closed after an error.  A family without the hooks
  // keeps the defaults, and begin throws as the guided and recorder calls do.
  // The ARENA is a mode of this one driver (pgx_arena.hip.h): SelfplayBegin with a second net.  A ply then writes the
  // side bytes of its leaf rows after the session's begin (ArenaSides), NetRunPairCall stands in place of NetRunCall,
  // and the tally keeps seven counters; everything else is the same calls.
  virtual bool HasSelfplay() const { return false; }
  virtual void SelfplayNoise(const SelfplayArgs& a);
  virtual void SelfplayMove(const SelfplayArgs& a);
  virtual void SelfplayTally(const SelfplayArgs& a);
  virtual void ArenaSides(const SelfplayArgs& a);
  // PUCT exploration (pgx_dirichlet.hip.h): `extra` (null: {0, 0, 1, 0}, the plain driver) adds Dirichlet root noise,
  // one launch (SelfplayDirichlet) between the round's first evaluation and its first advance, and a move temperature.
  // SelfplayNoiseRows: the host copy of the last ply's noise rows [N][A] (eta; a Gumbel driver: its Gumbel rows).
  virtual void SelfplayDirichlet(const SelfplayArgs& a);
  void SelfplayBegin(Net& net, const SelfplayOptions& o, Net* net_b = nullptr, const char* what = "selfplay_begin",
                     const SelfplayExtra* extra = nullptr);
  void SelfplayNoiseRows(float* out);
  void SelfplayRun(int plies, bool device);
  void SelfplayStats(int64_t out[6]);  // games, wins0, wins1, draws, plies, t
  void ArenaStats(int64_t out[8]);     // games, wins0, wins1, draws, plies, wins_a, wins_b, t: an arena only
  void SelfplayEnd();

 protected:
  // Family hook of the snapshot's last section: bytes per env of whatever the flat state does not carry, and the
  // kernel that packs (unpack: restores) it for the listed local envs, row i at d_buf + i * ExtraBytes(), on stream_.
  virtual size_t ExtraBytes() const { return 0; }
  virtual void PackExtra(const int* d_ids, int k, void* d_buf, bool unpack);
  // Launch the family's batched step kernel for k rows on stream_.
  // d_ids == nullptr means rows 0..k-1 map to local envs 0..k-1.
  virtual void Launch(const int* d_ids, int k, const void* d_action,
                      bool force_reset, const OutPtrs& out) = 0;
  void InitCommon();  // allocates + initialises CommonDev (after derived ctor)
  // device memory that lives as long as the pool: zeroed on `s` (default stream_), freed by ~Pool after every
  // stream has drained -- also when the derived constructor throws
  template <class T>
  T* DevAlloc(size_t count, hipStream_t s = nullptr) {
    void* p = DevMalloc(sizeof(T) * count);
    EPA_HIP(hipMemsetAsync(p, 0, sizeof(T) * count, s ? s : stream_));
    return static_cast<T*>(p);
  }
  // the same for a table: holds a copy of host[0, count), complete on return
  template <class T>
  T* DevUpload(const T* host, size_t count) {
    void* p = DevMalloc(sizeof(T) * count);
    EPA_HIP(hipMemcpy(p, host, sizeof(T) * count, hipMemcpyHostToDevice));
    return static_cast<T*>(p);
  }
  int WaveSlots();  // SIMDs of the device: one wave per SIMD, four SIMDs per CU (queried at the first call)
  // Per-pool error word for families whose kernels can meet a condition they must not spin on (a bounded
  // rejection loop that ran out): `err_dev_` is a pinned, device-mapped word the kernel stores a nonzero
  // code into; every recv that has waited for its rows' kernel (recv, recv_block, recv_into, and recv_device
  // for kernels already finished) then throws std::runtime_error(ErrorText(code)).  The word is sticky.
  void EnableErrorWord();
  virtual std::string ErrorText(unsigned code) const;
  unsigned* err_dev_{nullptr};
  // Generic TypedFrameStackBuffer (envpool/mujoco/frame_stack.h:74-146) for families
  // whose step kernel writes one un-stacked float64 observation per row: the first
  // env key must be "obs" declared with shape [S, nobs] (StackedObsShape).  The
  // kernel then writes into a scratch [k, nobs] block and a second small kernel
  // maintains a per-env ring and emits the stacked rows.  No-op for S == 1.
  void EnableObsStack();

  Config cfg_;
  std::vector<KeySpec> keys_;
  KeySpec action_;
  bool needs_rng_;
  // words of one env's generator kept contiguous (1 or 16; engine key "mt_tile" overrides): 1 for
  // families whose envs all draw at the same launches (the word a wave reads is one coalesced column), 16 for
  // families whose envs reset at their own times (a reset's draws then stay inside a few 64-byte sectors)
  int mt_tile_default_{1};
  // default of "step_pipeline" (see Pool::SendPipelined): 0 unless the family's constructor says otherwise -- it pays
  // where a step kernel takes about as long as its results need for the way down (the planar MuJoCo tasks: +18 %)
  // and costs where the kernel dominates (Ant: two half launches have two tails, -10 %)
  int pipeline_default_{0};
  // default of "direct_out" (Pool::SendInto): whether a whole-pool host-path step writes its results straight into
  // the block the caller named at send time (1), and also reads its action rows in place out of the pinned staging
  // slot instead of an uploaded copy (2: every family but the Ant, whose units would read them five times over)
  int direct_default_{2};
  // The stream the NEXT step kernel goes on.  Sync mode (batch_size == num_envs): always
  // compute_[0].  Async mode: successive batches rotate over the compute streams so that
  // independent in-flight batches run concurrently, like the reference's workers run every queued
  // slice in parallel (envpool/core/async_envpool.h:116-132); see PickStream.
  hipStream_t stream_{nullptr};
  hipStream_t h2d_stream_{nullptr};   // action uploads of the host path
  hipStream_t d2h_stream_{nullptr};   // result downloads of the host path
  // a pipelined step's big sections by DMA: first half on stream 2, second half on stream 3 (the small ones by a
  // gather kernel on d2h_stream_ / the kernel stream)
  hipStream_t d2h_stream2_{nullptr}, d2h_stream3_{nullptr};
  CommonDev common_{};

 private:
  // Rows the next Recv returns.  BLOCKS (mu_ released) until that many rows are pending -- AsyncEnvPool::Recv /
  // StateBufferQueue::Wait of the reference block on a semaphore (envpool/core/async_envpool.h:169-181,
  // state_buffer_queue.h:148-163), so a consumer thread may call recv before the producer's send.  Engine key
  // "recv_timeout_ms": < 0 (default) wait forever like the reference, 0 raise at once, > 0 raise after that long.
  int WantRows(std::unique_lock<std::mutex>& lk);
  void CopyRowsToHost(char* dst, const std::vector<size_t>& off, int want, std::unique_lock<std::mutex>& lk);
  Batch* AcquireBatch(int k);
  void ReleaseBatch(Batch* b);
  OutPtrs PtrsOf(const Batch& b) const;
  void Enqueue(const int* d_ids, int k, const void* d_action, bool force);
  Batch* BeginBatch(int k);
  // one launch of the family's step kernel for rows [row0, row0 + kp) of batch b
  void LaunchPart(Batch* b, const int* d_ids, int row0, int kp, const void* d_action, bool force);
  void FinishBatch(Batch* b);
  struct Staging;
  void SendPipelined(Staging& s, int k, const void* action, size_t id_bytes, size_t act_bytes,
                     char* direct_block);
  void SendImpl(const int32_t* env_id, int k, const void* action, char* block, size_t block_bytes);
  // a direct batch's rows [consumed, consumed + take) for recv: waits for its kernel, copies only if `dst` is not the
  // block the kernel wrote (CopyRowsToHost / RecvInto)
  void TakeDirect(Batch* b, int take, int got, char* dst, const size_t* dst_off, void* const* dst_ptrs,
                  std::unique_lock<std::mutex>& lk);
  void* DevMalloc(size_t bytes);   // hipMalloc, entered in dev_owned_
  std::vector<void*> dev_owned_;   // DevAlloc / DevUpload: freed by ~Pool, by nobody else
  int n_simd_{0};                  // WaveSlots (0: not asked yet)
  int direct_out_{-1};  // "direct_out" (-1: not read yet)
  unsigned* err_host_{nullptr};  // EnableErrorWord
  void CheckErrorWord() const;
  bool HostBlockVisible(const void* p);
  // chooses stream_ for the next launch and orders it behind what it may depend on
  void PickStream(const int32_t* host_ids, int k, bool device_path, const void* d_env_id = nullptr);
  void EnsureDone(Batch* b);  // records b->done on the batch's stream if nobody has yet
  void JoinCompute(hipStream_t into);  // `into` waits for everything enqueued on every compute stream
  void SyncCompute();                  // host waits for every compute stream
  void MarkIdle(Batch* b, int first, int count);
  struct Staging {
    char* h{nullptr};
    char* d{nullptr};
    size_t bytes{0};
    hipEvent_t free_ev{nullptr};   // the kernel that read this slot has finished
    hipEvent_t h2d_ev{nullptr};    // the upload into this slot has finished
    bool in_use{false};
  };
  Staging& NextStaging(size_t bytes);

 protected:
  void CheckIds(const int32_t* ids, int k) const;      // 0 <= k <= num_envs, then CheckIdRange
  void CheckIdRange(const int32_t* ids, int k) const;  // every id inside [env_id_offset, env_id_offset + num_envs)

 private:
  // generic observation frame stack (EnableObsStack)
  int stack_s_{1}, stack_nobs_{0};
  double* stack_ring_{nullptr};  // [N][S][nobs]
  int* stack_head_{nullptr};     // [N] slot holding the oldest frame
  double* stack_tmp_{nullptr};   // [N][nobs] un-stacked obs of the current launch
  std::mutex mu_;
  std::mutex recv_mu_;               // recv is single-consumer (state_buffer_queue.h:143-147): callers are serialised
  std::condition_variable pending_cv_;  // signalled by Enqueue; WantRows waits on it
  int recv_timeout_ms_{-1};
  int pipeline_rows_{-1};            // "step_pipeline": whole-pool host-path steps of at least this many rows (0: never)
  // [num_envs] GLOBAL env ids in order (SendPipelined: the second half's id list; a step launch takes the ids as the
  // caller sent them).  Not side_iota_, whose ids are local: with an env_id_offset the two tables differ
  int* iota_dev_{nullptr};
  int zero_copy_small_{-1};          // "small_zero_copy" (-1: not read yet)
  bool ZeroCopySmall() {
    if (zero_copy_small_ < 0) zero_copy_small_ = cfg_.Get("small_zero_copy", 1) != 0 ? 1 : 0;
    return zero_copy_small_ == 1;
  }
  std::unique_ptr<HostCopier> copier_;  // "copy_threads" helpers (default 2, 0 = none) for pipelined steps
  std::deque<Batch*> pending_;
  std::vector<std::vector<Batch*>> free_;  // per compute stream
  std::vector<std::unique_ptr<Batch>> all_;
  Batch* lent_[2]{nullptr, nullptr};  // batches handed out by RecvDevice
  std::vector<Staging> staging_;
  size_t staging_next_{0};
  char* recv_stage_{nullptr};  // pinned D2H landing block
  size_t recv_stage_bytes_{0};
  hipEvent_t order_ev_{nullptr};  // WaitStream's producer marker
  // Side operations: a call that reads or writes the state of listed envs outside the step path (get_state /
  // set_state, render, snapshot / restore / fork) is one launch on stream_ between these pieces; the caller holds mu_.
  // Ids are global, from the host.
  //   SideEnter    selects the device and puts the call behind the steps enqueued on the other compute streams: the
  //                host waits for them (host forms, which end in ONE hipStreamSynchronize(stream_)), or stream_ does
  //                (device forms, which end in SideLeave)
  //   SideIds      the launch's local ids on the device: the iota table for offset, offset + 1, ... (nothing to
  //                upload), otherwise a pinned + device slot, two in rotation; k may exceed num_envs (render)
  //   SideScratch  the pool's one device scratch block, at least that big, grow-only
  //   SideLeave    device forms: the other compute streams' next steps wait for what was enqueued here
  // The scratch block is shared by all of them although stream_ rotates between calls.  That is correct only because
  // every user enters through SideEnter -- so the previous user's work, on whichever stream, is ordered before this
  // one's -- and either synchronises stream_ or leaves through SideLeave before it releases mu_.
  void SideEnter(bool host_waits);
  const int* SideIds(const int32_t* ids, int k);
  char* SideScratch(size_t bytes);
  void SideLeave();
  int* side_iota_{nullptr};  // [num_envs] LOCAL ids 0, 1, ... (iota_dev_ holds global ones)
  struct IdSlot {
    int* h{nullptr};
    int* d{nullptr};
    int cap{0};
    hipEvent_t ev{nullptr};  // the upload out of `h` has finished
    bool used{false};
  };
  IdSlot side_slot_[2];
  int side_next_{0};
  hipEvent_t side_ev_{nullptr};  // behind the last device-form launch (SideLeave)
  char* side_scratch_{nullptr};
  size_t side_scratch_bytes_{0};
  void StateHost(const int32_t* ids, int k, double* out, const double* in);  // GetStateHost / SetStateHost
  // render's checks and the resolved size; throws before anything is enqueued
  void CheckRender(const int32_t* ids, int k, const void* out, int width, int height, int* w, int* h) const;
  // snapshots
  snap::PoolDesc SnapPoolDesc() const;  // what a header has to fit (snapshot.hip.h)
  void SnapCheck(const int32_t* ids, int k, bool unique) const;  // "not implemented", ids, duplicates
  void SnapPack(const int* d_ids, int k, unsigned flags, char* d_blob, void* host_header);
  void SnapUnpack(const int* d_ids, int k, const char* d_blob, const void* header);
  // playout's checks; throws before anything is enqueued
  void CheckPlayout(const int32_t* ids, int k, int repeats, int max_plies, unsigned flags) const;
  // search's checks; throws before anything is enqueued.  Returns the bytes of the tree scratch.
  size_t CheckSearch(const int32_t* ids, int k, int simulations, int leaf_playouts, float c_puct, int max_plies) const;
  // the checks of a solve call, before any launch; returns the bytes of the stacks (the tables follow them:
  // k * SolveTableBytes(table_bits))
  size_t CheckSolve(const int32_t* ids, int k, int depth, long long max_nodes, int table_bits) const;
  // the pool's guided-search session
  struct GuidedSession {
    bool open{false};
    DeviceBlock mem;        // the session's one device allocation: roots, nodes, the host forms' staging, and with
                            // tactics the counters and the solver's stacks
    char* pinned{nullptr};  // the host forms' pinned block, laid out like the staging
    bool gumbel{false};     // the session's policy: PUCT or Gumbel
    int k{0}, simulations{0}, calls{0};
    int width{0};           // slots per root of a wide PUCT session; 0: a plain session
    int batch{0};           // slots per root of a batch Gumbel session; 0: a plain session
    int capacity{0};        // nodes per root (PUCT: simulations + 1 .. EPA_GUIDED_MAX_NODES; Gumbel: simulations + 1)
    float c_puct{0.0f};
    int considered{0};      // Gumbel: m, c_visit, c_scale
    float c_visit{0.0f}, c_scale{0.0f};
    size_t nodes_off{0}, stage_off{0};
    int tactics{0};         // exact leaf status: D (0: off), M, and the offset of its block behind the staging:
    long long tactics_nodes{0};  // decided int32 [k], nodes int64 [k], then the slots' stacks
    size_t tactics_off{0};
    int flags{0};           // EPA_GUIDED_PROVE: proven values; its read-out's staging (int8 [k] and [k][A]) is the
    size_t proof_off{0};    // allocation's last block
    // offsets into the staging: priors (Gumbel: the noise at begin, then logits), values, obs, mask, status, visits,
    // vals, action, the end of a PUCT session's staging, and behind it a Gumbel session's weights and their end
    size_t off[10]{};
  };
  GuidedSession guided_;
  void GuidedFree();                                   // (no session: nothing)
  // A begin's block of `bytes`: an open session's block of exactly that size is kept -- no free and no allocation, so
  // the begin does not wait for the device (a self-play driver begins once per ply); any other is released first.
  // Result-neutral: a begin initialises what it reads.
  void GuidedReserve(size_t bytes);
  void GuidedRequire(const char* what) const;          // throws without a session
  void GuidedRequirePolicy(const char* what, bool gumbel) const;  // ... or with one of the other policy
  // what GuidedArgs and GumbelArgs share: the session's sizes, call number, roots and nodes, and for a host form the
  // staging arrays, `rows` among them (the caller's rows of an advance: priors or logits)
  template <class Args>
  Args SessionArgsOf(bool device, const float* Args::*rows) const;
  GuidedArgs GuidedArgsOf(bool device) const;          // the session's pointers; staging arrays for a host form
  TacticsArgs TacticsArgsOf() const;                   // (a session with tactics)
  GumbelArgs GumbelArgsOf(bool device) const;
  // One session call in either form, between SideEnter and SideLeave; `launch` enqueues the call's work on stream_.
  //   device form  launch, SideLeave: nothing waits
  //   host form    bytes [up.lo, up.hi) of the pinned block go to the staging, launch, bytes [down.lo, down.hi) of the
  //                staging come back to the pinned block, ONE hipStreamSynchronize(stream_); an empty range: no copy
  // The caller fills SessionPinned() before and reads it after; its checks come before both.
  struct StageRange {
    size_t lo{0}, hi{0};
  };
  template <class Launch>
  void SessionRun(bool device, StageRange up, StageRange down, Launch launch);
  char* SessionPinned();  // the host forms' pinned block, allocated at its first use in a session
  // the pool's recorder
  struct Recorder {
    bool open{false};
    DeviceBlock mem;        // the recorder's one device allocation, in the order of `off`
    char* pinned{nullptr};  // the host forms' rows: policy [N][A], reward [N][2], done [N]; then int64 [5] for reads
    int capacity{0}, plies{0}, nsym{1};
    int32_t shape[4]{};     // H, W, C, A
    // offsets into mem: states, elapsed, staged policy, n_e, plan, count + counters + item count (64 bytes), the seven
    // sample arrays, the device copies of the host forms' rows (policy, reward, done), finish's item list, the end
    size_t off[18]{};
  };
  Recorder record_;
  void RecordFree();                                    // (no recorder: nothing)
  void RecordRequire(const char* what) const;           // throws without the hooks or without a recorder
  RecordArgs RecordArgsOf(int k) const;
  void RecordCheckIds(const char* what, const int32_t* ids, int k) const;  // range, count, repeats
  // the pool's rollout collector
  struct Rollout {
    bool open{false};
    bool started{false};    // RolloutReset has run
    DeviceBlock mem;        // the collector's one device allocation, in the order of `off`
    int horizon{0}, capacity{0}, t{0};
    unsigned flags{0};
    long long step{0};
    std::vector<int> obs_keys;      // indices into keys_
    std::vector<int> moment_keys;   // positions in obs_keys of the float keys
    std::vector<int> moment_comp0;  // their first component
    int comps{0};
    std::vector<size_t> obs_off;    // per obs key
    // offsets into mem: action, reward, term, trunc, mask, carry + acc_ret + acc_len (one zeroed run), emit, emit_ret,
    // emit_len, the four episode arrays, the control words, the moment accumulators and partials, the staged action
    // and values / adv / ret rows of the host forms, the end
    size_t off[22]{};
  };
  Rollout rollout_;
  void RolloutFree();
  void RolloutRequire(const char* what) const;
  void RolloutQuiet(const char* what) const;     // throws unless the result queue is empty
  RolloutStepArgs RolloutArgsOf(const Batch& b) const;
  void RolloutMomentsOf(int slot);               // enqueues the moment kernels for one obs slot
  // the collector's actor
  struct Actor {
    bool open{false};
    DeviceBlock mem;        // the actor's one device allocation, in the order of `off`
    NetImage image;
    int F{0}, H{0}, kind{0};
    unsigned flags{0};
    uint64_t seed{0};
    // offsets into mem: the net image, lo, scale, sigma, low, high, the feature rows [N][F], the head's rows
    // [N][H + 1], logp [T][N], value [T+1][N], the end
    size_t off[11]{};
  };
  Actor actor_;
  void ActorFree();
  void ActorRequire(const char* what) const;     // throws without a collector or without an actor
  int ActorFeatures() const;                      // F of the pool: the components of the collector's obs keys
  // enqueues features -> trunk -> sample for `rows` rows on stream_: obs key j's rows at src[j]
  void ActorEnqueue(const char* const* src, int rows, const int32_t* d_env_id, long long step, bool value_only,
                    unsigned char* features, int32_t* head, void* action, float* logp, float* value);
  // the pool's self-play driver
  struct Selfplay {
    bool open{false};
    DeviceBlock mem;        // the driver's one device allocation, in the order of `off`
    Net* net{nullptr};
    Net* net_b{nullptr};    // an arena: the net of side 1
    SelfplayOptions o{};
    SelfplayExtra x{0.0f, 0.0f, 1.0f, 0};
    size_t noise_bytes{0};  // of the noise rows [N][A]
    uint32_t t{0};          // the ply counter
    std::vector<int32_t> ids;  // the pool's global ids in order
    // offsets into mem: noise, obs, mask, status (the leaf arrays, one row per root or slot), visits, vals, result
    // action, weights, the action row, the target rows, the counters (64 bytes), the side bytes (an arena: one per
    // leaf row), the end
    size_t off[13]{};
  };
  Selfplay selfplay_;
  int NetRunImpl(Net& net, Net* net_b, int advances, void* obs, void* mask, void* status, const void* side,
                 bool device, const char* what, const NetRunHook* after_first);  // NetRunCall and NetRunPairCall
  void SelfplayFree();                                  // (no driver: nothing)
  void SelfplayPly();                                   // one ply, enqueued
  uint64_t family_hash_{0};
  // concurrent batches (async mode)
  std::vector<hipStream_t> compute_;     // compute_[0] is the sync-mode stream
  std::vector<hipEvent_t> join_ev_;      // one per compute stream (JoinCompute)
  size_t rr_{0};
  bool picked_{false};                   // WaitStream already chose the stream of the next launch
  std::vector<uint32_t> busy_;           // host path: rows of this env launched and not received yet (a count)
  std::vector<Batch*> frontier_;         // device path: batches handed out whose kernels may still run
  const int32_t* next_host_ids_{nullptr};  // ids of the launch being enqueued (for Batch::host_ids)
  bool next_identity_{false};
  // timing
  int timing_{0};
  hipEvent_t win0_{nullptr}, win1_{nullptr};  // timing mode 2: first launch .. KernelTime()
  bool win_open_{false};
  int win_launches_{0};
  std::vector<std::pair<hipEvent_t, hipEvent_t>> timers_;
  std::vector<hipEvent_t> timer_pool_;
};

// Where the flat state of a gym-MuJoCo pool lives on the device.  The flat state is the one oracle/mjcpu uses:
//   qpos[nq] qvel[nv] warm[nv] | time xlag ylag done cur_step normal_saved normal_avail [| lag[lag_rows]]
// GetState writes all of it, SetState takes everything but `time`; done is stored as (x != 0), cur_step as
// (int)x, normal_avail as (x != 0).  A part a family does not have reads 0 and is ignored on SetState:
//                                    time (read only)               xlag ylag                  normal_saved / _avail
//   HalfCheetah, Walker2d            Newton iterations, last step   -                          yes
//   Hopper (3 ghost rows)            Newton iterations, last step   -                          yes
//   Ant                              profiling counters, last step  lagged torso x, y          yes
//   Inverted(Double)Pendulum         -                              -                          yes
//   Swimmer                          -                              -                          yes (never drawn from)
//   Reacher                          -                              lagged fingertip x, y      -
//   Humanoid, HumanoidStandup        -                              lagged mass centre x, y    -
//   Pusher                           -                              copies of lag rows 0, 1    -
// The Pusher has five lag rows (xpos of tips_arm, x / y of the object, of the last forward evaluation): they follow
// the common part as lag[5], SetState takes them from there and ignores xlag / ylag.
struct MjStateView {
  double* qpos;  // [nq + ghost][N]
  double* qvel;  // [nv + ghost][N]
  double* warm;  // [nv + ghost][N]
  int nq, nv;    // as they appear in the flat state
  // the optional parts
  int ghost{0};            // rows the device arrays have beyond that (the Hopper's second leg): SetState zeroes them
  double* lag{nullptr};    // [lag_rows][N]
  int lag_rows{0};         // 0, 2 (xlag ylag), or more (appended)
  double* nsaved{nullptr};         // [N], with
  unsigned char* navail{nullptr};  // [N]
  const int* time_i{nullptr};      // [N] what `time` reports: one of the two, or neither (0)
  const double* time_d{nullptr};
};

// A pool whose state hooks are the flat state of its view; the family fills view_ from the pointers it steps.
class MjPool : public Pool {
 public:
  using Pool::Pool;
  int StateDim() const override;
  void GetState(const int* d_ids, int k, double* d_out) override;
  void SetState(const int* d_ids, int k, const double* d_in) override;

 protected:
  MjStateView view_{};  // (a copy of pointers the family's own *Dev struct holds: the step kernels take that)
};

// Diagnostic per-wave trace of a family's step kernel: when the environment variable
// `env` names a file, `d` is a device buffer of 6 x int64 per wave that the kernel fills
// (wall clock begin / end at 100 MHz, core clock begin / end, two family-specific words)
// and the buffer of the LAST launch is written to that file when the pool is destroyed
// (tools/ant_trace_stats.py, tools/planar_trace_stats.py).  Off (d == nullptr) otherwise.
struct WaveTrace {
  long long* d{nullptr};
  size_t waves{0};
  std::string file;
  void Init(const char* env, size_t n_waves, hipStream_t s);
  void DumpAndFree();
};

// obs key shape with the optional leading frame_stack dimension (StackSpec,
// envpool/mujoco/frame_stack.h:42-71); throws like the reference on frame_stack < 1
std::vector<int> StackedObsShape(const Config& cfg, int nobs);

// The family table (engine.hip), one row per name in epa_family_name order.  A family file exports one
// describe / make pair and is only ever called with the names its rows give it; describe must accept any config
// (epa_describe_* pass the caller's params alone, epa_family_players a default Config).
struct Family {
  const char* name;
  FamilySpec (*describe)(const std::string& name, const Config& cfg);
  Pool* (*make)(const std::string& name, const Config& cfg);
};
const std::vector<Family>& Families();
const Family& FindFamily(const std::string& name);  // throws invalid_argument("unknown env family: " + name)

FamilySpec DescribeClassicControl(const std::string& name, const Config& cfg);
Pool* MakeClassicControl(const std::string& name, const Config& cfg);
FamilySpec DescribeToyText(const std::string& name, const Config& cfg);
Pool* MakeToyText(const std::string& name, const Config& cfg);
FamilySpec DescribeMujocoGym(const std::string& name, const Config& cfg);  // HalfCheetah, Walker2d, Hopper
Pool* MakeMujocoGym(const std::string& name, const Config& cfg);
FamilySpec DescribeAnt(const std::string& name, const Config& cfg);
Pool* MakeAnt(const std::string& name, const Config& cfg);
// InvertedPendulum, InvertedDoublePendulum, Reacher, Swimmer
FamilySpec DescribePendulum(const std::string& name, const Config& cfg);
Pool* MakePendulum(const std::string& name, const Config& cfg);
FamilySpec DescribeHumanoid(const std::string& name, const Config& cfg);  // Humanoid, HumanoidStandup
Pool* MakeHumanoid(const std::string& name, const Config& cfg);
FamilySpec DescribePusher(const std::string& name, const Config& cfg);
Pool* MakePusher(const std::string& name, const Config& cfg);
FamilySpec DescribeMiniGrid(const std::string& name, const Config& cfg);
Pool* MakeMiniGrid(const std::string& name, const Config& cfg);
FamilySpec DescribeJumanji(const std::string& name, const Config& cfg);
Pool* MakeJumanji(const std::string& name, const Config& cfg);
FamilySpec DescribePgx(const std::string& name, const Config& cfg);
Pool* MakePgx(const std::string& name, const Config& cfg);
// Atari (atari_env.hip) is not in the table: it needs two strings the numeric epa_config cannot carry
Pool* MakeAtari(const Config& cfg, const std::string& rom_path, const std::string& emulator_lib);
int AtariNumActions(const Config& cfg, const std::string& rom_path, const std::string& emulator_lib);

void SetLastError(const std::string& msg);  // thread-local epa_last_error()

// Launch helpers shared by the family files.
void LaunchInitCommon(CommonDev c, int seed, const int* d_env_seed,
                      int id_offset, bool with_rng, hipStream_t s);

}  // namespace epa

#endif  // ENVPOOL_AMD_CSRC_ENGINE_H_
