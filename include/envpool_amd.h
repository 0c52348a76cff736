/*
 * envpool_amd — C ABI of the MI355X-native batched-step engine.
 *
 * This is the drop-in boundary for ONE path of sail-sg/envpool: the batched
 * Send()/Recv()/Reset() execution path.  In the reference that path is the
 * C++ virtual class `EnvPool<Spec>` (envpool/core/envpool.h:29-56) implemented
 * by `AsyncEnvPool<Env>` (envpool/core/async_envpool.h:42-238: thread pool +
 * ActionBufferQueue + StateBufferQueue) and bound to Python by
 * `PyEnvPool<Pool>` (envpool/core/py_envpool.h:206-288).  Here the thread pool
 * and the queues are replaced by device-resident SoA env state and one batched
 * HIP kernel per env family; everything above (`PySend/PyRecv/PyReset`, the
 * Python adaptors) can stay and bind to the functions below
 * (see INTEGRATION.md for the pybind11 / ctypes stubs).
 *
 * Conventions
 *  - every function returns 0 on success, non-zero on failure;
 *    `epa_last_error()` then holds a message (thread local).  Error classes
 *    follow the reference: EPA_ERR_INVALID  <-> std::invalid_argument
 *    (-> Python ValueError, envpool/core/env_spec.h:75-80), EPA_ERR_RUNTIME <->
 *    std::runtime_error (-> RuntimeError).
 *  - plain pointers and sizes only; no C++/torch types.
 *  - arrays are C-contiguous, row-major, one row per env in the batch.
 *  - key order is the reference's (envpool/core/env_spec.h:32-43):
 *      actions: "env_id", "players.env_id", <env action keys...>
 *      states : "info:env_id", "info:players.env_id", "elapsed_step", "done",
 *               "reward", "discount", "step_type", "trunc", <env state keys...>
 */
#ifndef ENVPOOL_AMD_H_
#define ENVPOOL_AMD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EPA_OK 0
#define EPA_ERR_INVALID 1 /* std::invalid_argument in the reference */
#define EPA_ERR_RUNTIME 2 /* std::runtime_error in the reference */
#define EPA_ERR_DEVICE 3  /* HIP failure (no reference analogue) */

/* element types of state / action arrays */
#define EPA_I32 0
#define EPA_F32 1
#define EPA_F64 2
#define EPA_BOOL 3 /* 1 byte, numpy bool_ */
#define EPA_U8 4
#define EPA_I8 5 /* int8 (Jumanji RubiksCube obs:cube) */

typedef struct epa_pool epa_pool;

/*
 * Pool configuration = the reference's `common_config`
 * (envpool/core/env_spec.h:26-31) restricted to what the step path reads, plus
 * per-family numeric options passed as (key, value) pairs named exactly like
 * the reference's `XxxEnvFns::DefaultConfig()` keys (e.g. "version" for
 * Pendulum, "size" for FrozenLake, "frame_skip", "ctrl_cost_weight", ...).
 * Unknown keys are ignored.  Engine extensions (not reference keys):
 *   "precision"   Ant: 1 fp64 (default), 0 fp32 arithmetic (meets 1e-5).  HalfCheetah / Walker2d / Hopper: only 1
 *                 (their fp32 mode was removed in round 4: outside 1e-5 and slower than the fp64 kernel)
 *   "xml_v5"      Walker2d / Pusher: 1 selects the *_v5 model (the reference's xml_file)
 *   "planar_spread" HalfCheetah / Walker2d / Hopper / Pusher: 1 (default) a batch of 16 .. 64 (Pusher: 32 .. 64) envs
 *                 per SIMD is spread over all SIMDs with 16 / 32 / 48 envs per wave; 0 always 64 envs per wave
 *   "hum_layout"  Humanoid / HumanoidStandup: 1 one env per lane quad (default), 0 one env per lane -- the superseded
 *                 kernel, built only into lib/libenvpool_amd_alt.so (`make -C envpool_amd/csrc EPA_ALT_KERNELS=1`, the
 *                 cross-check tests load it through ENVPOOL_AMD_LIB); the product library refuses 0
 *   "hum_sort"    quad layout: 1 cost-sorted waves (default), 0 rows in send order
 *   "hum_debug"   quad layout: stages switched off (bits 1 2 4 8), solver statistics (16) or cycles per stage
 *                 (32 64 128 256) routed into the info keys; accepted by the diagnostic build only
 *                 (-DEPA_HUM_DEBUG: tools/build_trace_lib.sh, tools/build_alt_hum4.sh), the product library refuses it
 *   "planar_layout" HalfCheetah / Walker2d, fp64: lanes per env of the step kernel -- 2 or 4 (one env per
 *                 lane group, mujoco_planar_lg.hip), 1 (one env per lane, mujoco_gym.hip), 0 (default)
 *                 chosen once per pool: 2 above 16384 rows, else 4 (rows = num_envs in sync mode,
 *                 min(num_envs, 4 x batch_size) in async mode: what is in flight on the compute streams).
 *                 The two layouts sum the contact rows in different orders: with the default, an env's
 *                 low-order bits therefore depend on the pool's num_envs / batch_size (never on the rows
 *                 of a particular send); set the key explicitly where pools of different shape must agree
 *                 bit for bit.  Each layout is within 1e-9 of the oracle per env-step.
 *                 Hopper: 0 (default) the lane-group kernel with a group of ONE lane (the lane's 6 dofs are
 *                 the robot), 1 the one-env-per-lane kernel on the 9-dof tree with a ghost leg; 2 / 4 refused.
 *   "planar_waves" lane-group kernel with 4 lanes per env: register budget for 1 (default) or 2 waves per SIMD
 *                 (A/B switch; with 1 or 2 lanes per env LDS allows one wave and the key has no effect)
 *   "planar_lpt"  lane-group kernel: 1 whole-pool launches serve the chunks of envs slowest first, by their
 *                 duration in the previous launch (default for Walker2d / Hopper); 0 index order (default for
 *                 HalfCheetah since round 5).  Never changes results.
 *   "step_pipeline" sync pools, host path (epa_send): a whole-pool send of at least this many rows runs as TWO launches
 *                 over the two halves of the rows, and epa_recv* downloads the first half while the second computes (the
 *                 rows still arrive as ONE batch in send order, every value bit-identical to the single launch).
 *                 Default 32768 for HalfCheetah / Walker2d pools with 2 lanes per env (where half the rows take half
 *                 the time: numpy API +20 %), 0 = off for every other family (measured slower there); 0 switches it off.
 *   "copy_threads" helper threads (default 2, 0 .. 8) that copy the action rows of a pipelined step into the pinned
 *                 staging slot together with the calling thread; they poll ~0.3 ms after a step, then sleep
 *   "direct_out"  what epa_send_into does for a whole-pool step of a sync pool: 0 = it is epa_send; 1 = the step
 *                 kernel writes its rows straight into the caller's block; 2 (default; the Ant: 1) = that, and the
 *                 action rows are read in place out of the pinned staging slot (no upload): numpy step of HalfCheetah
 *                 N = 65536 0.46 -> 0.43 ms, Hopper 0.48 -> 0.39, Pusher 0.87 -> 0.65.  Never changes results.
 *   "small_zero_copy" 1 (default): host-path batches of up to 64 KB go without DMA commands -- the step kernel reads ids
 *                 and action rows straight out of the pinned staging slot, epa_recv's landing block is filled by a copy
 *                 kernel on the kernel stream (CartPole num_envs = 64: send + recv 32.4 -> 29.4 us); 0 = DMA as for
 *                 bigger batches.  Never changes results.
 *   "numa_bind"   1 (default): those helper threads run on the CPUs of the device's NUMA node (where this runtime
 *                 allocates pinned memory); 0 leaves them to the scheduler.  The CALLING thread is never moved by the
 *                 library: envpool_amd.bind_host_to_device() (Python) does that for a process that wants it, as the
 *                 reference's benchmark/numa_test.sh does with numactl
 *   "ant_sub"     Ant: mj_steps per unit of the step kernel's work queue (default 1: an env-step of a 16-env chunk is
 *                 frame_skip units, the chunk's state goes through HBM between them; frame_skip = one unit per chunk,
 *                 the schedule of rounds 2-5; a sub that does not divide frame_skip makes the last unit of an
 *                 env-step shorter).  Never changes results.
 *   "selftest"    MuJoCo families with a self-test table (HalfCheetah, Walker2d, Hopper, Ant, Humanoid,
 *                 HumanoidStandup): 0 skips the load-time self-test for this pool (see epa_create); the environment
 *                 variable EPA_SELFTEST=0 skips it for the process
 *   "classic_block", "classic_rows" classic_control: threads per block (64 / 128 / 256, default by family and size) and
 *                 rows per thread of the step kernel (A/B keys; never change results)
 *   "classic_early" classic_control: 1 = the step kernel reads state, action and generator position together with
 *                 `done`, in front of the reset branch (default: CartPole only, where every wave holds a reset row:
 *                 -6 % kernel time at num_envs = 65536); never changes results
 *   "mt_tile"     every family with generators: consecutive words of ONE env's mt19937 that are kept contiguous in device
 *                 memory -- 1 = the plain [624][N] structure of arrays (every env draws the same word in the same
 *                 launch: a draw is one coalesced column), 16 = tiles of 16 words per env, [39][N][16] (envs that reset
 *                 at their own times: a reset's 8 .. 60 draws stay inside 1 .. 4 64-byte sectors).  Default by family:
 *                 16 where episodes end at their own times (CartPole, Acrobot, FrozenLake, Taxi, Blackjack, Walker2d,
 *                 the Ant, Humanoid, the inverted pendulums, Jumanji, MiniGrid, PGX), 1 elsewhere; any other value is
 *                 refused.  Never changes results: both layouts produce std::mt19937's sequence, and a snapshot taken
 *                 in one restores into a pool built with the other.
 *   "recv_timeout_ms" every family: how long epa_recv* waits for rows that have not been sent yet (see epa_recv):
 *                 < 0 forever (default, the reference's behaviour), 0 not at all, > 0 milliseconds
 *   "compute_streams" async mode (batch_size < num_envs): successive batches run on this many
 *                 compute streams (default 4, 1 = one stream), like the reference's worker threads
 *                 step all queued slices in parallel (core/async_envpool.h:116-132).  Pools with the generic
 *                 frame stack (frame_stack > 1) and the one-env-per-lane Humanoid kernel (hum_layout = 0, one
 *                 shared workspace) keep one stream.  Device memory of the Humanoid quad pools' per-launch scratch:
 *                 compute_streams x W(batch_size) + W(num_envs), W(rows) = 1.9 MB per 16 rows (the second term only
 *                 once a send exceeds batch_size rows, e.g. the reset of all envs; such sends share one copy and are
 *                 ordered behind each other).  A device-path send whose env ids do not continue a handed-out batch
 *                 (identity ids, ids from elsewhere) is ordered behind EVERY batch still executing or pending.
 *                 The rule for the caller is the reference's: an env may be sent
 *                 again only after recv handed it out (host path: a violation is detected and that
 *                 launch is ordered behind everything enqueued; device path: the env ids of a send
 *                 should be the `info:env_id` array of a batch recv_device returned -- the launch then
 *                 continues that batch's stream -- any other pointer is ordered behind every batch
 *                 still executing).
 */
typedef struct epa_config {
  int32_t num_envs;          /* common_config "num_envs" */
  int32_t batch_size;        /* "batch_size"; 0 => num_envs (env_spec.h:81-83) */
  int32_t seed;              /* "seed": env i is seeded seed + i (env.h:109) */
  const int32_t* env_seed;   /* "env_seed": NULL or num_envs explicit seeds */
  int32_t max_episode_steps; /* "max_episode_steps"; <=0 => INT_MAX */
  int32_t device;            /* HIP device ordinal (extension) */
  int32_t env_id_offset;     /* global id of local env 0 when a pool is one
                                shard of a multi-GPU pool (extension) */
  int32_t n_params;
  const char* const* param_keys;
  const double* param_values;
} epa_config;

/* One state or action key. `shape` excludes the leading batch dimension.
 * Single-player families (epa_family_players == 1) drop the reference's -1
 * player dimension.  A family of P > 1 players (the PGX board games) keeps it
 * as the leading P of the per-row shape of its per-player state keys
 * ("info:players.env_id", "reward", "discount" and the family's own per-player
 * keys, see epa_describe_state_players): a batch of k rows then holds the
 * reference's k * P player rows as a [k, P, ...] block, env-major, which is
 * the reference's [k * P, ...] layout.  Actions stay one row per env. */
typedef struct epa_key_info {
  const char* name;
  int32_t dtype;
  int32_t ndim;
  int32_t shape[4];
  int32_t row_elems; /* product of shape (1 for scalars) */
  int32_t row_bytes;
} epa_key_info;

/* ---- spec queries: no GPU needed ------------------------------------- */

/* Number of env families compiled in and their names ("CartPole", ...). */
int epa_num_families(void);
const char* epa_family_name(int i);

/* Describe the state/action keys a family would produce for `cfg`
 * (replaces EnvSpec<Fns>::{state_spec,action_spec}, env_spec.h:48-85).
 * Writes up to `cap` entries; returns the total number through *n. */
int epa_describe_state(const char* family, const epa_config* cfg,
                       epa_key_info* keys, int cap, int* n);
int epa_describe_action(const char* family, const epa_config* cfg,
                        epa_key_info* keys, int cap, int* n);

/* Number of players P of a family (1 for every single-player family). */
int epa_family_players(const char* family, int32_t* players);
/* Per state key (epa_describe_state order): P if the key's rows carry the
 * leading player dimension, 1 otherwise.  Writes up to `cap` entries; returns
 * the total number through *n. */
int epa_describe_state_players(const char* family, const epa_config* cfg,
                               int32_t* players, int cap, int* n);

/* ---- pool lifetime ---------------------------------------------------- */

/* Replaces AsyncEnvPool<Env>::AsyncEnvPool(spec) (async_envpool.h:90-149):
 * allocates SoA state for num_envs envs on `cfg->device`, seeds every env's
 * mt19937 (env.h:101-117) and marks every env done so that the first step is a
 * reset (cartpole.h:67 `done_{true}`, async_envpool.h:127).
 * The FIRST pool of a MuJoCo family in a process (per device) also runs the library's self-test: fixed states are
 * stepped once in every kernel variant of the family and compared with the same arithmetic evaluated on the host at
 * build time (envpool_amd/csrc/gen_selftest.cpp), and the launch is repeated and must be bit-identical; a library that
 * was not built the way envpool_amd/csrc/Makefile builds it is refused with EPA_ERR_DEVICE (~25 ms; EPA_SELFTEST=0 or
 * the engine key "selftest" = 0 skip it). */
int epa_create(const char* family, const epa_config* cfg, epa_pool** out);

/* Replaces ~AsyncEnvPool (async_envpool.h:151-162). */
int epa_destroy(epa_pool* pool);

/* ---- host path: the reference's Send / Recv / Reset -------------------- */

/* Replaces AsyncEnvPool::Send(vector<Array>) (async_envpool.h:59-82,163-167).
 * `env_id[k]` int32, `action` = k rows of the family's action key in its
 * reference dtype.  Copies both into pinned staging (the caller may free its
 * buffers on return), enqueues H2D + one batched step kernel on the pool's
 * stream and returns immediately.  Row i of the resulting batch belongs to
 * env_id[i] (sync-mode ordering, state_buffer.h:94-97). */
int epa_send(epa_pool* pool, const int32_t* env_id, int32_t k,
             const void* action);

/* Replaces AsyncEnvPool::Reset(env_ids) (async_envpool.h:224-237): forced
 * reset of the listed envs; the result arrives through epa_recv. */
int epa_reset(epa_pool* pool, const int32_t* env_ids, int32_t k);

/* Replaces AsyncEnvPool::Recv() (async_envpool.h:169-181).  Blocks until the
 * oldest pending rows are computed, copies them device->host into
 * `out_ptrs[key]` (one buffer per state key, each with room for `cap_rows`
 * rows) and returns the number of rows through *k_out.
 *   sync  mode (batch_size == num_envs): returns the whole oldest send/reset
 *         batch (k rows, possibly < num_envs for a partial env_id send).
 *   async mode (batch_size <  num_envs): returns exactly batch_size rows in
 *         completion (= submission) order, a legal schedule of
 *         state_buffer_queue.h:123-163.
 * BLOCKS, like the reference (StateBufferQueue::Wait sits on a semaphore, state_buffer_queue.h:148-163; the binding
 * releases the GIL around it, py_envpool.h:255-262): a consumer thread may call epa_recv BEFORE the producer thread's
 * epa_send / epa_reset -- it returns once enough rows have been enqueued and computed.  send / reset from other
 * threads are not held up by a waiting or downloading consumer.  recv itself is single-consumer
 * (state_buffer_queue.h:143-147): concurrent calls are serialised.  Extension key "recv_timeout_ms" (epa_config
 * params): < 0 (default) wait forever; 0 EPA_ERR_RUNTIME at once when fewer rows are pending than a batch holds (for
 * single-threaded callers that would otherwise hang); > 0 EPA_ERR_RUNTIME after that many milliseconds.
 * epa_recv_block / epa_recv_into / epa_recv_device / epa_step_device wait the same way. */
int epa_recv(epa_pool* pool, void* const* out_ptrs, int32_t n_ptrs,
             int32_t cap_rows, int32_t* k_out);

/* Zero-copy variant of epa_recv: the reference hands numpy arrays that OWN
 * their memory and are never overwritten by later steps (py_envpool.h:40-49,
 * state_buffer_queue.h:149-163: a fresh buffer per batch).  Here the caller
 * provides one host block per batch (pinned memory from epa_host_alloc gives the
 * full PCIe rate), the batch lands in it with ONE device->host copy and no host
 * memcpy, and the per-key arrays are views at `offsets[key]`.
 * epa_recv_layout: section offsets (256-B aligned) and total size of a block
 * holding `rows` rows of every state key.
 * epa_recv_block: same blocking / batching semantics as epa_recv; `offsets`
 * (n_keys entries) is filled for the *k_out rows actually returned. */
int epa_recv_layout(epa_pool* pool, int32_t rows, size_t* offsets, int32_t n_keys,
                    size_t* total_bytes);
int epa_recv_block(epa_pool* pool, void* block, size_t block_bytes,
                   size_t* offsets, int32_t n_keys, int32_t* k_out);

/* epa_send for a caller that already knows WHERE the results shall go (the reference's StateBufferQueue allocates the
 * batch's output buffers before the workers write them, state_buffer_queue.h:123-140): `block` is a pinned host block
 * (epa_host_alloc) with room for k rows laid out by epa_recv_layout(k), which stays the caller's but must live until
 * the epa_recv_block that returns this batch.  For a batch that recv will return as a whole -- every env of a sync pool,
 * or batch_size rows of an async pool -- the
 * step kernel then writes its rows STRAIGHT into the block -- they cross the link as the kernel's own stores, while
 * it runs -- and epa_recv_block with the same block only waits for the kernel (any other recv call copies out of the
 * block).  By default it also reads the action rows in place out of the pinned staging slot: no DMA command at all in
 * such a step.  A send whose block is too small or not pinned, or with the extension key "direct_out" = 0, behaves
 * exactly like epa_send and ignores the block; rows that a recv returns in pieces or together with other batches'
 * rows are copied out of the block.  Results are the same bytes either way. */
int epa_send_into(epa_pool* pool, const int32_t* env_id, int32_t k, const void* action, void* block,
                  size_t block_bytes);

/* Same blocking / batching semantics as epa_recv, but every state key is copied
 * device->host DIRECTLY into `out_ptrs[key]` (no landing block, no host memcpy;
 * pinned destinations get the full PCIe rate, NULL skips a key).  This is the
 * building block of the multi-GPU host gather: GPU g's rows land
 * in ITS row range of one host batch shared by all GPUs. */
int epa_recv_into(epa_pool* pool, void* const* out_ptrs, int32_t n_ptrs,
                  int32_t cap_rows, int32_t* k_out);

/* Rows currently computed-or-in-flight and not yet received. */
int epa_pending_rows(epa_pool* pool, int32_t* rows);

/* ---- device path (zero-copy; the analogue of envpool/core/xla.h:116-213
 *      without the host staging the reference does there) ---------------- */

/* Like epa_send but `d_env_id` (may be NULL = all envs in order) and
 * `d_action` (NULL = forced reset of the listed envs) are device pointers on
 * the pool's device.  The step kernel is enqueued on the pool's stream behind
 * `wait_event` (a hipEvent_t as void*, may be NULL) -- the event the producer
 * of the action buffer recorded on ITS stream after writing it.  This is the
 * stream-ordering half of the reference's XLA custom call
 * (envpool/core/xla.h:151-169), minus its host staging.  With NULL the caller
 * must have made the buffers visible some other way (epa_wait_stream below, or
 * a device synchronise). */
int epa_send_device(epa_pool* pool, const int32_t* d_env_id, int32_t k,
                    const void* d_action, void* wait_event);

/* Convenience for callers that have a stream rather than an event (e.g.
 * torch.cuda.current_stream().cuda_stream): everything enqueued on
 * `producer_stream` (hipStream_t as void*; NULL = the legacy default stream)
 * so far happens-before every kernel the pool enqueues from now on. */
int epa_wait_stream(epa_pool* pool, void* producer_stream);

/* Hands out device pointers (one per state key) to the oldest pending batch.
 * The pointers stay valid until the second next epa_recv_device call on this
 * pool (batches are double buffered).  Does not synchronise the host: work
 * enqueued on epa_stream() after this call is ordered after the step kernel. */
int epa_recv_device(epa_pool* pool, void** d_out_ptrs, int32_t n_ptrs,
                    int32_t* k_out);

/* epa_send_device followed by epa_recv_device in ONE call -- the device-path form of the reference's sync `step()`
 * (envpool/python/envpool.py:345-349: send, then recv).  At the sizes where a step kernel takes a few microseconds
 * (classic_control / toy_text at num_envs = 65536) the two calls of a binding are most of a step's time. */
int epa_step_device(epa_pool* pool, const int32_t* d_env_id, int32_t k, const void* d_action,
                    void* wait_event, void** d_out_ptrs, int32_t n_ptrs, int32_t* k_out);

/* The mirror of epa_wait_stream for the outputs: `consumer_stream` waits for the
 * step kernel of the batch the LAST epa_recv_device handed out (a consumer on
 * epa_stream() itself needs no call).  The consumer must be done with a batch's
 * buffers before the second next epa_recv_device, when they are recycled. */
int epa_consumer_wait(epa_pool* pool, void* consumer_stream);

/* hipStream_t of the pool, as void*. */
void* epa_stream(epa_pool* pool);
int epa_synchronize(epa_pool* pool);

/* Average duration in ms of the step kernels launched since the last call,
 * measured with HIP events on the pool's stream; *launches = how many.
 * epa_set_timing(pool, 1): an event pair around every launch (exact per-launch
 * durations; the events keep consecutive launches ~12 us apart).
 * epa_set_timing(pool, 2): one event before the first launch and one when
 * epa_kernel_time_ms is called: (elapsed / launches), inter-launch gaps included,
 * nothing inserted between the launches -- what bench.py uses for its timed region.
 * epa_set_timing(pool, 0): off. */
int epa_set_timing(epa_pool* pool, int32_t enabled);
int epa_kernel_time_ms(epa_pool* pool, double* avg_ms, int32_t* launches);

/* Test hooks: read / overwrite the persistent state of the listed envs as the
 * family's flat double vector (CartPole: x,x_dot,theta,theta_dot; HalfCheetah:
 * qpos[9],qvel[9],qacc_warmstart[9],time ...).  Mirrors the reference's
 * ENVPOOL_TEST-only `info:qpos0/qvel0` state sync
 * (envpool/mujoco/gym/half_cheetah.h:50-53,112-115). */
int epa_state_dim(epa_pool* pool, int32_t* dim);
int epa_get_state(epa_pool* pool, const int32_t* env_ids, int32_t k,
                  double* out);
int epa_set_state(epa_pool* pool, const int32_t* env_ids, int32_t k,
                  const double* in);

/* Replaces AsyncEnvPool::Render (async_envpool.h:183-222, render_mode "rgb_array"): uint8 [k, H, W, 3] row-major
 * RGB frames of the listed envs, painted on the device from their persistent state, byte-identical with the
 * reference's RenderableEnv::Render.  Families: the six Jumanji puzzles and the four PGX board games; every other
 * family fails with EPA_ERR_RUNTIME "render not implemented for this environment", like an env of the reference that
 * is no RenderableEnv.
 *   width / height <= 0: the env's default (256 x 256; TicTacToe 192 x 192, ConnectFour 280 x 240, Hex 352 x 352);
 *     epa_render_size resolves them the same way, so the caller can size its buffer.  A side above 4096 is refused.
 *   camera_id: accepted and ignored, as in the reference.
 *   env_ids: global ids (env_id_offset included), any count >= 1, duplicates allowed.  EPA_ERR_INVALID for k <= 0
 *     ("render env_ids must not be empty") and for an id outside the pool (as epa_get_state).
 * A frame shows its env after every send / reset issued before the call, received or not; a finished env shows its
 * terminal state until its next step resets it.  Rendering changes nothing a later send or recv sees.
 * epa_render returns the frames in host memory.  epa_render_device writes them to device memory of the pool's
 * device (any alignment) and copies nothing to the host: it only enqueues, stream-ordered like epa_recv_device --
 * order the consumer behind epa_stream(pool), and call epa_wait_stream first if the buffer is still in use on
 * another stream. */
int epa_render_size(epa_pool* pool, int32_t width, int32_t height, int32_t* w, int32_t* h);
int epa_render(epa_pool* pool, const int32_t* env_ids, int32_t k, int32_t width, int32_t height, int32_t camera_id,
               uint8_t* host_out);
int epa_render_device(epa_pool* pool, const int32_t* env_ids, int32_t k, int32_t width, int32_t height,
                      int32_t camera_id, void* device_out);

/* Snapshot, restore and fork (no reference analogue): everything that makes the listed envs continue bit for bit, as
 * one opaque blob -- a 64-byte header (magic, version, hash of the family name, state_dim, env count, flags, generator
 * layout, frame stack, byte count), the flat state of epa_get_state, with EPA_SNAP_RNG the 624 generator words and the
 * position of every env, and the observation ring of frame_stack > 1.  A pool restored from a snapshot with
 * EPA_SNAP_RNG returns the same rows as the pool the snapshot was taken from, resets and their draws included; without
 * the flag a restore leaves the target's generators alone (what epa_set_state does, plus the observation ring).
 *   env_ids: global ids, k >= 1; a restore's ids and a fork's dst_ids must not repeat (EPA_ERR_INVALID).
 *   A snapshot shows each env after every send / reset issued before the call, received or not; a restore takes
 *   effect before every send issued after it and leaves rows already waiting for recv alone.
 *   A blob may be restored into any pool of the same family with the same state_dim and frame_stack, whatever its
 *   seed, size or engine keys; EPA_ERR_INVALID when the header does not fit the pool or the ids, or the blob is
 *   shorter than its header says (the blob's body is read only after that).
 *   Atari (the console lives in the host plugin) fails with EPA_ERR_RUNTIME "snapshot not implemented for this
 *   environment" in all six calls.
 * epa_snapshot / epa_restore move the blob to / from host memory: one copy across and one stream synchronisation.
 * epa_snapshot_device / epa_restore_device work on device memory of the pool's device (16-byte aligned, at least
 * epa_snapshot_bytes) and only enqueue on epa_stream(pool), like epa_render_device; host_header (64 bytes of host
 * memory) receives the header from epa_snapshot_device (NULL: not wanted) and hands it back to epa_restore_device,
 * which checks it without reading device memory.
 * epa_fork: env dst_ids[i] becomes env src_ids[i], on the device; src_ids may repeat and may overlap dst_ids. */
#define EPA_SNAP_RNG 1u
int epa_snapshot_bytes(epa_pool* pool, int32_t k, uint32_t flags, size_t* bytes);
int epa_snapshot(epa_pool* pool, const int32_t* env_ids, int32_t k, uint32_t flags, void* host_blob,
                 size_t blob_bytes);
int epa_restore(epa_pool* pool, const int32_t* env_ids, int32_t k, const void* host_blob, size_t blob_bytes);
int epa_snapshot_device(epa_pool* pool, const int32_t* env_ids, int32_t k, uint32_t flags, void* device_blob,
                        void* host_header);
int epa_restore_device(epa_pool* pool, const int32_t* env_ids, int32_t k, const void* device_blob,
                       const void* host_header);
int epa_fork(epa_pool* pool, const int32_t* src_ids, const int32_t* dst_ids, int32_t k, uint32_t flags);

/* Random playouts (no reference analogue; the four PGX board games): every listed env is played on `repeats` times
 * from its current state -- the state after every send / reset issued before the call, received or not, as for
 * epa_snapshot -- with uniformly drawn legal actions, until its game is over or max_plies plies are played
 * (max_plies = 0: EPA_PLAYOUT_MAX_PLIES, which no game of the four reaches).  One kernel launch, one playout per lane,
 * no result rows.  The draws (all arithmetic mod 2^64):
 *   SM(x):  x += 0x9E3779B97F4A7C15; x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9;
 *           x = (x ^ (x >> 27)) * 0x94D049BB133111EB; return x ^ (x >> 31)
 *   stream  h = SM(seed ^ SM((uint64(env_id) << 32) | uint32(r)))       env_id: the global id; r: the repeat, from 0
 *   ply t   (from 0 inside the playout)  u = SM(h + t); n = legal actions; j = ((u >> 32) * n) >> 32;
 *           the action is the (j+1)-th lowest legal one
 * so a playout depends on (seed, env_id, r) and the position only, not on the order of the ids or on how the pool
 * is sharded.  Results, entry i * repeats + r for env_ids[i]'s repeat r:
 *   returns [k, repeats, 2] float   per-player sum of the step rewards (0 and +-1: exact)
 *   plies   [k, repeats]    int32   plies played
 *   status  [k, repeats]    uint8   0 the game is over, 1 stopped at max_plies
 * An env that is over at the call (every env before its first reset is) reports 0 plies, zero returns and status 0;
 * a playout never resets an env.  By default nothing of the pool changes: not the envs, their step counts and
 * generators, nor the rows waiting for recv.  With EPA_PLAYOUT_COMMIT (repeats = 1, ids that do not repeat) the final
 * state is written back, done set and the step count advanced by `plies`, exactly as if those actions had been stepped
 * except that no rows are produced; it takes effect before every send issued after the call, like epa_restore.
 *   EPA_ERR_INVALID: repeats outside 1 .. EPA_PLAYOUT_MAX_REPEATS, max_plies outside 0 .. EPA_PLAYOUT_MAX_PLIES,
 *     unknown flags, k <= 0, more than num_envs ids or an id outside the pool (global ids, as epa_snapshot), k * repeats
 *     above 2^31 - 1, commit with repeats != 1 or with a repeated id.
 *   Every other family fails with EPA_ERR_RUNTIME "playout not implemented for this environment".
 * epa_playout returns the results in host memory (one stream synchronisation).  epa_playout_device writes them to
 * device memory of the pool's device (returns 8-byte, plies 4-byte aligned) and only enqueues on epa_stream(pool),
 * like epa_snapshot_device. */
#define EPA_PLAYOUT_COMMIT 1u
#define EPA_PLAYOUT_MAX_PLIES 256
#define EPA_PLAYOUT_MAX_REPEATS 4096
int epa_playout(epa_pool* pool, const int32_t* env_ids, int32_t k, int32_t repeats, int32_t max_plies, uint64_t seed,
                uint32_t flags, float* returns, int32_t* plies, uint8_t* status);
int epa_playout_device(epa_pool* pool, const int32_t* env_ids, int32_t k, int32_t repeats, int32_t max_plies,
                       uint64_t seed, uint32_t flags, void* device_returns, void* device_plies, void* device_status);

/* Tree search (no reference analogue; the four PGX board games): for every listed env, `simulations` (S) rounds of PUCT
 * selection from its current state -- the state after every send / reset issued before the call, as for epa_snapshot --
 * with uniform priors, every new leaf valued by the sum of `leaf_playouts` (R) uniform-random playouts.  One kernel
 * launch, one wave per root; nothing of the pool changes and no result rows are produced.  The contract, with e the
 * root's GLOBAL env id (csrc/pgx_search.hip.h):
 *   A node holds its position, term0 (seat 0's reward of the step that made it) and per action a: child[a] (-1: none),
 *   v[a] (simulations through the edge), w0[a] (seat 0's summed playout returns through the edge), all int32.  Node 0
 *   is the env's position; a root has at most S + 1 nodes.
 *   simulation t = 0 .. S-1:
 *     node = 0; path = []
 *     loop:
 *       if node's game is over:  val0 = R * node.term0; break
 *       a = the legal action of the largest score(node, a); ties: the lowest a
 *       path += (node, a)
 *       if node.child[a] < 0:
 *           c = a new node: node's position stepped by a, term0 = seat 0's reward of that step; node.child[a] = c
 *           if c's game is over:  val0 = R * c.term0
 *           else:  val0 = sum over r < R of seat 0's return of repeat t * R + r of epa_playout(seed, env e, max_plies)
 *                         played from c's position
 *           break
 *       node = node.child[a]
 *     for (n, a) in path:  n.v[a] += 1;  n.w0[a] += val0
 *   score(node, a), float, every operation correctly rounded, in this order, nothing fused:
 *     V = sum over b of node.v[b];  sign = +1 if seat 0 moves at the node else -1   (the seat info:current_player reports)
 *     q = node.v[a] > 0 ? (float)(sign * node.w0[a]) / (float)(node.v[a] * R) : 0
 *     score = q + (c_puct * sqrtf((float)V)) / (float)(1 + node.v[a])
 * Only seat 0's value is kept: legal play in the four games is zero-sum with step rewards 0 and +-1.  Results, row i
 * for env_ids[i], A the game's number of actions:
 *   visits  [k, A] int32   the root's v
 *   returns [k, A] int32   the root's w0, times the sign of the root's mover
 *   action  [k]    int32   the action with most visits; ties: the lowest
 * Illegal root actions have visits 0 and returns 0.  An env that is over at the call (every env before its first reset
 * is) reports zeros and action -1.  A result depends on (seed, e, S, R, c_puct, max_plies) and the position only, not
 * on the order of the ids or on how the pool is sharded.
 *   EPA_ERR_INVALID: S outside 1 .. EPA_SEARCH_MAX_SIMULATIONS, R outside 1 .. EPA_SEARCH_MAX_LEAF_PLAYOUTS,
 *     S * R above EPA_PLAYOUT_MAX_REPEATS, max_plies outside 0 .. EPA_PLAYOUT_MAX_PLIES, c_puct not finite or negative,
 *     k <= 0, more than num_envs ids or an id outside the pool (global ids, as epa_snapshot), and a tree scratch
 *     (k * (S + 1) nodes) above EPA_SEARCH_MAX_TREE_BYTES: the message names the largest k that fits.
 *   Every other family fails with EPA_ERR_RUNTIME "search not implemented for this environment".
 *   A position that is no position of the game (a running game without a legal action) sets the pool's error word:
 *   epa_search and the next recv fail with EPA_ERR_RUNTIME, and that root's rows are those of an env that is over.
 * epa_search_actions gives A, the width of a result row (0 for a family without search).
 * epa_search returns the results in host memory (one stream synchronisation).  epa_search_device writes them to device
 * memory of the pool's device (4-byte aligned) and only enqueues on epa_stream(pool), like epa_snapshot_device. */
#define EPA_SEARCH_MAX_SIMULATIONS 4096
#define EPA_SEARCH_MAX_LEAF_PLAYOUTS 64
#define EPA_SEARCH_MAX_TREE_BYTES 2147483648ull
int epa_search_actions(epa_pool* pool, int32_t* out);
int epa_search(epa_pool* pool, const int32_t* env_ids, int32_t k, int32_t simulations, int32_t leaf_playouts,
               float c_puct, int32_t max_plies, uint64_t seed, int32_t* visits, int32_t* returns, int32_t* action);
int epa_search_device(epa_pool* pool, const int32_t* env_ids, int32_t k, int32_t simulations, int32_t leaf_playouts,
                      float c_puct, int32_t max_plies, uint64_t seed, void* device_visits, void* device_returns,
                      void* device_action);

/* PGX solve (no reference analogue; the four PGX board games): the exact minimax value of every listed env's current
 * position -- the state after every send / reset issued before the call, as for epa_snapshot -- per root action, by
 * alpha-beta in one kernel launch, one wave per root.  No model, no random numbers; nothing of the pool changes and no
 * result rows are produced.  The contract (csrc/pgx_solve.hip.h), D = depth, A = the game's number of actions:
 *   D = 0 means no horizon, up to EPA_SOLVE_MAX_DEPTH plies (a whole Hex or Othello game fits).  T_D(root) is the game
 *   tree from the root, cut after D plies.  A leaf that is a finished game has the value of its last step's reward for
 *   the mover at the root (+1, 0, -1); a leaf cut by the horizon has value 0; interior values are plain minimax, an
 *   Othello pass and Hex's swap being plies like any other.  Results, row i for env_ids[i]:
 *     value  [k]    int8    the maximum of q over the legal actions
 *     q      [k, A] int8    per legal root action the minimax value of T_D through it, seen from the root's mover;
 *                           -128 for an illegal action
 *     action [k]    int32   the lowest legal action whose q equals value
 *     status [k]    uint8   0 solved; 1 given up: more than max_nodes positions were visited for this root, or a line
 *                           went past EPA_SOLVE_MAX_DEPTH plies; 2 the env is over at the call (every env before its
 *                           first reset is).  A row with status 1 or 2 has value 0, action -1 and q -128 throughout.
 *     nodes  [k]    int64   the positions visited
 *   With D > 0, value +1 means a forced win within D plies, -1 a forced loss within D plies, 0 neither: the tactical
 *   check of bounded cost.  D = 0 gives the game-theoretic value.
 *   The values are exact and so independent of the traversal.  `nodes`, and which rows are given up at a tight
 *   max_nodes, depend on it (max_nodes is looked at between rounds of 512 positions per lane, so a row that is given
 *   up reports somewhat more than max_nodes; a solved row never does); for them the contract is determinism: the same
 *   call gives the same bytes, and a row depends on its position, D and max_nodes only, not on the order of the ids,
 *   repeated ids or how the pool is sharded.
 *   EPA_ERR_INVALID, before any launch: D outside 0 .. EPA_SOLVE_MAX_DEPTH, max_nodes < 1, k <= 0, more than num_envs
 *     ids or an id outside the pool (the id checks of epa_search), and stacks (k roots x 64 lanes x D plies, D = 0:
 *     EPA_SOLVE_MAX_DEPTH, x 80 bytes) above EPA_SEARCH_MAX_TREE_BYTES: the message names the largest k that fits.
 *   Every other family fails with EPA_ERR_RUNTIME "solve not implemented for this environment".
 *   A position that is no position of the game (a running game without a legal action) sets the pool's error word:
 *   epa_solve and the next recv fail with EPA_ERR_RUNTIME, and that root's row is given up.
 * A row is epa_search_actions wide.  epa_solve returns the results in host memory (one stream synchronisation).
 * epa_solve_device writes them to device memory of the pool's device (action 4-byte, nodes 8-byte aligned) and only
 * enqueues on epa_stream(pool), like epa_search_device. */
#define EPA_SOLVE_MAX_DEPTH 128
int epa_solve(epa_pool* pool, const int32_t* env_ids, int32_t k, int32_t depth, int64_t max_nodes, int8_t* value,
              int8_t* q, int32_t* action, uint8_t* status, int64_t* nodes);
int epa_solve_device(epa_pool* pool, const int32_t* env_ids, int32_t k, int32_t depth, int64_t max_nodes,
                     void* device_value, void* device_q, void* device_action, void* device_status,
                     void* device_nodes);

/* PGX solve with transposition tables (csrc/pgx_solve.hip.h "Transposition tables"): epa_solve / epa_solve_device with
 * table_bits = b, 0 .. EPA_SOLVE_MAX_TABLE_BITS.
 *   b = 0: exactly epa_solve / epa_solve_device (which call these entries with 0): the same launches and the same
 *     bytes in all five results.
 *   b > 0: every lane of a root's wave owns a private table of 2^b entries of 32 bytes in device memory, empty at the
 *     start of every call (the engine clears the buffer on the pool's stream) and kept over the frontier entries the
 *     lane takes.  It stores a lower and an upper bound of every finished position with at least two plies left to
 *     the horizon (D = 0: to the cap), and a position that Step just made is looked up before it is searched.  A hit
 *     needs the whole position, the plies left included, to be equal; the hash only picks the slot.
 *   value, q, action and status 0 / 2 are those of epa_solve wherever both solve the row: the values are exact.
 *   `nodes` is mostly smaller (no promise per row), and which rows are given up at a tight max_nodes follows the new
 *   traversal.  Determinism as for epa_solve: the same call gives the same bytes, and a row depends on its position,
 *   D, max_nodes and b only -- the tables are private to a lane, so not on id order, repeated ids or sharding.
 *   EPA_ERR_INVALID, before any launch, beside the refusals of epa_solve: b outside 0 .. EPA_SOLVE_MAX_TABLE_BITS
 *     ("solve: table_bits = .. must be in 0 .. 16"); the stacks plus the tables (k roots x 64 lanes x 2^b x 32 bytes)
 *     above EPA_SEARCH_MAX_TREE_BYTES: the message names the largest k that fits. */
#define EPA_SOLVE_MAX_TABLE_BITS 16
int epa_solve_table(epa_pool* pool, const int32_t* env_ids, int32_t k, int32_t depth, int64_t max_nodes,
                    int32_t table_bits, int8_t* value, int8_t* q, int32_t* action, uint8_t* status, int64_t* nodes);
int epa_solve_table_device(epa_pool* pool, const int32_t* env_ids, int32_t k, int32_t depth, int64_t max_nodes,
                           int32_t table_bits, void* device_value, void* device_q, void* device_action,
                           void* device_status, void* device_nodes);

/* Guided tree search (no reference analogue; the four PGX board games): a PUCT search whose tree lives on the device
 * between calls and that stops at every new leaf, so that the caller -- a policy / value model next to the pool in
 * HBM -- supplies the priors and the leaf values (AlphaZero-style).  One kernel launch per simulation, one wave per
 * root; no random numbers anywhere.  The contract (csrc/pgx_guided.hip.h), S = simulations, A = the game's actions:
 *   A SESSION belongs to one pool and covers the k listed roots; a root has up to S + 1 nodes.  A node holds its
 *   position, term0 (seat 0's reward of the step that made it) and per action a: child[a] (-1: none), v[a] (int32
 *   visits), w0[a] (float, seat 0's summed value through the edge), p[a] (float prior).  Per root the session keeps the
 *   node count, the PENDING LEAF, its status and the current path of (node, action) pairs.
 *   status 0: evaluate this leaf; 1: the leaf is a finished game, its value is known and the caller's row is ignored;
 *          2: nothing is pending (the root was over at begin, or the session has used all its simulations).
 *   begin(ids, S, c_puct):
 *     per root: node 0 = the env's position; path = []; pending = 0; status = 2 if the env is over else 0
 *     emit leaves.
 *   advance(priors[k, A], values[k]) -- call number t = 0 .. S:
 *     per root with status != 2, L = pending:
 *       status 0: for every a: L.p[a] = clean(priors[i, a]);  val0 = sign(L) * cleanv(values[i])
 *       status 1: val0 = (float) L.term0
 *       for (n, a) in path:  n.v[a] += 1;  n.w0[a] += val0            (float add)
 *       if t == S:  status = 2
 *       else:  node = 0; path = []
 *         loop:
 *           a = the legal action of the largest score(node, a); ties: the lowest a
 *           path += (node, a)
 *           if node.child[a] < 0:
 *               c = a new node: node's position stepped by a, term0 = seat 0's reward of that step
 *               node.child[a] = c;  node = c;  break
 *           node = node.child[a]
 *           if node's game is over: break
 *         pending = node;  status = 1 if node's game is over else 0
 *     emit leaves.
 *   score(node, a), float, every operation correctly rounded, in this order, nothing fused:
 *     V = sum over b of node.v[b];  sign = +1 if seat 0 moves at the node else -1
 *     q = node.v[a] > 0 ? (sign * node.w0[a]) / (float) node.v[a] : 0
 *     score = q + ((c_puct * node.p[a]) * sqrtf((float)(V + 1))) / (float)(1 + node.v[a])
 *   clean(x) = (x >= 0 && x <= FLT_MAX) ? x : 0       cleanv(x) = (x >= -1 && x <= 1) ? x : 0
 * values[i] is the leaf's value for the seat that moves there, the seat whose observation was emitted.  Priors are used
 * as given: the caller normalises them and mixes in root noise; entries of illegal actions are never read by a pick.
 * clean / cleanv give every bit pattern a defined result in the _device forms, which cannot look at their rows; the
 * host forms refuse such a row (any row, ignored ones included) with EPA_ERR_INVALID before any launch.
 * Emitted leaves -- epa_guided_begin and every epa_guided_advance write, for all k rows:
 *   obs    [k, H, W, C] bool   the observation of the seat that moves at the pending leaf, element for element what a
 *                              step into that position returns in that seat's "obs" row
 *   mask   [k, A]       bool   the position's legal-action mask
 *   status [k]          uint8
 * Rows of status 1 or 2 are all zeros in obs and mask.
 * epa_guided_result is valid any time after begin and complete after S + 1 advances:
 *   visits [k, A] int32   the root's v
 *   values [k, A] float   the root's w0 times the sign of the root's mover
 *   action [k]    int32   the most visited legal action, the lowest on ties; -1, and zero rows, for a root that was over
 * Session rules.  A pool has at most one session; a second begin replaces it.  begin sees the state after every send /
 * reset issued before it, as epa_snapshot does.  The session works on its own copies of the positions: stepping the
 * pool between advances changes nothing in the session, and the session changes nothing in the pool.  Its memory is
 * one device allocation owned by the pool -- not the scratch block epa_search, epa_render and epa_snapshot reuse --
 * released by epa_guided_end, by the next begin and by epa_destroy.  A result depends on the arguments, the positions
 * and the caller's numbers only: not on id order, repeated ids or sharding.
 *   EPA_ERR_INVALID, before any launch: S outside 1 .. EPA_SEARCH_MAX_SIMULATIONS; c_puct negative or not finite; the
 *     id checks of epa_search; trees (k * (S + 1) nodes) above EPA_SEARCH_MAX_TREE_BYTES: the message names the largest k
 *     that fits; advance, result or end without a session; a call number above S; priors / values of k != the session's
 *     rows.
 *   Every other family fails with EPA_ERR_RUNTIME "guided search not implemented for this environment".
 *   A position that is no position of the game (a running game without a legal action, or a path past the cap) ends
 *   that root with status 2 and sets the pool's error word, as for epa_search.
 * epa_guided_shape gives {H, W, C, A} (zeros for a family without guided search).
 * The host forms copy through pinned memory and synchronise once.  The _device forms take and write device pointers
 * of the pool's device (float and int32 arrays 4-byte aligned) and only enqueue on epa_stream(pool).  epa_guided_end
 * has one form: it moves no data. */
int epa_guided_shape(epa_pool* pool, int32_t* out);
int epa_guided_begin(epa_pool* pool, const int32_t* env_ids, int32_t k, int32_t simulations, float c_puct,
                     uint8_t* obs, uint8_t* mask, uint8_t* status);
int epa_guided_begin_device(epa_pool* pool, const int32_t* env_ids, int32_t k, int32_t simulations, float c_puct,
                            void* device_obs, void* device_mask, void* device_status);
int epa_guided_advance(epa_pool* pool, const float* priors, const float* values, int32_t k, uint8_t* obs,
                       uint8_t* mask, uint8_t* status);
int epa_guided_advance_device(epa_pool* pool, const void* device_priors, const void* device_values, int32_t k,
                              void* device_obs, void* device_mask, void* device_status);
int epa_guided_result(epa_pool* pool, int32_t* visits, float* values, int32_t* action);
int epa_guided_result_device(epa_pool* pool, void* device_visits, void* device_values, void* device_action);
int epa_guided_end(epa_pool* pool);

/* Guided search, tree reuse (PUCT sessions; csrc/pgx_guided.hip.h "Tree reuse" is the authority): after a move is
 * played, the subtree under it becomes the tree of the next search, so the simulations already evaluated below it are
 * not paid for again.
 *   CAPACITY.  A session has C nodes per root.  epa_guided_begin keeps C = S + 1, and a session that is never rerooted
 *   is byte for byte what it always was.  epa_guided_begin_nodes is epa_guided_begin with `nodes` = C,
 *   S + 1 <= C <= EPA_GUIDED_MAX_NODES; the trees are k * C nodes.  advance has one more rule: a root begins a descent
 *   only if its node count is below C; otherwise it goes to status 2 for the rest of the round -- a normal end, "memory
 *   used up", which sets no error.  With C = S + 1 and no reroot it never triggers.
 *   epa_guided_reroot(actions[k], S2) is allowed once the round is complete (S + 1 advances made).  Per root, a =
 *   actions[i]:
 *     a root that was over (or broken)  stays over; a is ignored
 *     a outside 0 .. A-1                the root is over (the host form refuses the row instead)
 *     node0.child[a] = c >= 0           the nodes reachable from c are kept and compacted in place: a kept node's new
 *                                       index is its rank among the kept ones in increasing old index (c becomes 0),
 *                                       child[] is remapped, every other field stays bit for bit; count = the number kept
 *     node0.child[a] < 0                node 0 = the root position stepped by a, no edges, count = 1
 *     then                              the new root's game is over (an illegal a ends the game, too): the root is over,
 *                                       status 2, and the result is -1 and zero rows; otherwise pending = node 0, status 0
 *   The session's simulations become S2 (1 .. EPA_SEARCH_MAX_SIMULATIONS, S2 + 1 <= C), the call number restarts at 0,
 *   and the leaves are emitted as begin emits them.  The new root is always handed out for evaluation: advance 0 of the
 *   new round stores the caller's priors into it (replacing the old ones) and backs up nothing; the statistics below it
 *   stay, and epa_guided_result counts the kept visits.  A round after reroot is again S2 + 1 advances for all roots.
 *   EPA_ERR_INVALID, before any launch: reroot without a session, on a Gumbel session ("reroot not implemented for
 *     gumbel sessions") or before the round's last advance; k != the session's rows; in the host form an action outside
 *     0 .. A-1; S2 outside 1 .. EPA_SEARCH_MAX_SIMULATIONS or S2 + 1 > C; nodes outside S + 1 .. EPA_GUIDED_MAX_NODES;
 *     trees above EPA_SEARCH_MAX_TREE_BYTES (the message names the largest k that fits).
 *   Every other family fails with EPA_ERR_RUNTIME "guided search not implemented for this environment".
 * The _device forms take device pointers (actions: int32 [k], 4-byte aligned) and only enqueue. */
#define EPA_GUIDED_MAX_NODES 8192
int epa_guided_begin_nodes(epa_pool* pool, const int32_t* env_ids, int32_t k, int32_t simulations, int32_t nodes,
                           float c_puct, uint8_t* obs, uint8_t* mask, uint8_t* status);
int epa_guided_begin_nodes_device(epa_pool* pool, const int32_t* env_ids, int32_t k, int32_t simulations,
                                  int32_t nodes, float c_puct, void* device_obs, void* device_mask,
                                  void* device_status);
int epa_guided_reroot(epa_pool* pool, const int32_t* actions, int32_t k, int32_t simulations, uint8_t* obs,
                      uint8_t* mask, uint8_t* status);
int epa_guided_reroot_device(epa_pool* pool, const void* device_actions, int32_t k, int32_t simulations,
                             void* device_obs, void* device_mask, void* device_status);

/* Guided search, several leaves per launch (PUCT sessions; csrc/pgx_guided.hip.h "Several leaves per launch" is the
 * authority): a WIDE session of width W, 1 .. EPA_GUIDED_MAX_WIDTH, keeps W slots per root -- each a pending leaf, a
 * status and a path -- and one advance answers every pending slot and then descends up to W times per root, the
 * descents steered apart by virtual losses, so that a move of S simulations costs about S / W + 1 model calls of
 * k * W rows instead of S + 1 calls of k rows.  Through this interface a wide session is a session of k * W rows: obs,
 * mask and status of begin, advance and reroot, and priors and values of advance, have k * W rows, row i * W + j for
 * slot j of root i; `k` of epa_guided_advance is k * W.  epa_guided_reroot still takes one action per root (its `k`
 * is the number of roots), and epa_guided_result gives one row per root, as for a plain session.
 *   A slot of status 2 has nothing pending and its rows are zeros.  A round is complete when all k * W statuses are 2,
 *   after at most S + 1 advances (typically about S / W + 1); later advances up to call number S change nothing, and a
 *   call number above S is refused.  A descent that arrives at a leaf handed out earlier in the same launch is dropped
 *   (a collision), and that root hands out no further leaf in that launch.  Width 1 is the plain session, call for call.
 *   `nodes`: the capacity per root, 0 for S + 1, as epa_guided_begin_nodes.
 *   epa_guided_reroot of a wide session: the host form refuses while any slot is pending; the device form cannot look:
 *   slots still pending are dropped and nothing of them is backed up -- finish the round first.  After it slot 0 of
 *   every root holds the new root and the other slots are idle.
 *   EPA_ERR_INVALID, before any launch, beside the refusals of epa_guided_begin_nodes: a width outside 1 ..
 *     EPA_GUIDED_MAX_WIDTH; advance with a row count other than k * W; a host reroot with a pending slot.  The tree
 *     limit EPA_SEARCH_MAX_TREE_BYTES counts the wide root records (about 1 KiB per slot).
 * The _device form takes device pointers and only enqueues. */
#define EPA_GUIDED_MAX_WIDTH 32
int epa_guided_begin_wide(epa_pool* pool, const int32_t* env_ids, int32_t k, int32_t simulations, int32_t nodes,
                          int32_t width, float c_puct, uint8_t* obs, uint8_t* mask, uint8_t* status);
int epa_guided_begin_wide_device(epa_pool* pool, const int32_t* env_ids, int32_t k, int32_t simulations,
                                 int32_t nodes, int32_t width, float c_puct, void* device_obs, void* device_mask,
                                 void* device_status);

/* Guided search, exact leaf status (PUCT sessions, plain or wide; csrc/pgx_guided.hip.h "Exact leaf status" is the
 * authority): a session begun with tactics = D, 1 .. EPA_GUIDED_MAX_TACTICS, hands every new leaf other than the root
 * to the exact solver (epa_solve's contract, unchanged: the tree of D plies from the leaf's position, max_nodes =
 * tactics_nodes, 1 .. EPA_GUIDED_MAX_TACTICS_NODES) after the advance's descents.  A leaf the solver decides -- status
 * solved, value v != 0 -- is from then on a finished game whose last reward is v for the seat that moves there: its
 * row has status 1 and zeros in obs and mask, the caller's row for it is ignored, and +-1 is backed up.  A value of 0
 * or a leaf given up is evaluated by the caller as before.  A decided node that a reroot makes the root runs on: it is
 * handed out with status 0.  Which leaves are decided does not depend on id order or sharding.
 *   width = 0: a plain session; 1 .. EPA_GUIDED_MAX_WIDTH: a wide one.  nodes = 0: simulations + 1.
 *   tactics = 0: exactly epa_guided_begin / _nodes / _wide: the same launches and the same bytes.
 *   epa_guided_decided: decided int32 [k], the leaves decided per root since begin (a reroot does not reduce it);
 *     nodes int64 [k] (may be null), the positions the solver visited per root since begin.  Zeros for a session
 *     without tactics.
 *   EPA_ERR_INVALID, before any launch, beside the refusals of epa_guided_begin_wide: tactics outside 0 ..
 *     EPA_GUIDED_MAX_TACTICS; tactics_nodes outside 1 .. EPA_GUIDED_MAX_TACTICS_NODES; the trees plus the solver's
 *     stacks (5120 bytes x D per slot) above EPA_SEARCH_MAX_TREE_BYTES: the message names the largest k that fits.
 * The _device forms take device pointers and only enqueue. */
#define EPA_GUIDED_MAX_TACTICS 16
#define EPA_GUIDED_MAX_TACTICS_NODES (1 << 20)
#define EPA_GUIDED_TACTICS_NODES 4096 /* the default of the Python layers */
int epa_guided_begin_tactics(epa_pool* pool, const int32_t* env_ids, int32_t k, int32_t simulations, int32_t nodes,
                             int32_t width, float c_puct, int32_t tactics, int64_t tactics_nodes, uint8_t* obs,
                             uint8_t* mask, uint8_t* status);
int epa_guided_begin_tactics_device(epa_pool* pool, const int32_t* env_ids, int32_t k, int32_t simulations,
                                    int32_t nodes, int32_t width, float c_puct, int32_t tactics,
                                    int64_t tactics_nodes, void* device_obs, void* device_mask, void* device_status);
int epa_guided_decided(epa_pool* pool, int32_t* decided, int64_t* nodes);
int epa_guided_decided_device(epa_pool* pool, void* device_decided, void* device_nodes);

/* Guided search, proven values (PUCT sessions, plain or wide, with or without nodes, tactics and reroot;
 * csrc/pgx_guided.hip.h "Proven values" is the authority; MCTS-Solver): a session begun with flags = EPA_GUIDED_PROVE
 * lets exact values climb the tree.  A finished game and a decided leaf are proven nodes; a node with a child proven +1
 * for its mover is proven +1, a node whose every legal move leads to a proven child is proven with the best of their
 * values (-1, 0 or +1), and such a node counts as finished from then on.  A pick never takes a move whose child is a
 * proven loss for the mover while another is left, a proven root begins no further descent (its rows have status 2 for
 * the rest of the round), and epa_guided_result's action is the most visited move that keeps the root's proven value,
 * or for an unproven root the most visited move not proven to lose.  visits and values are unchanged.
 *   epa_guided_begin_prove: the arguments of epa_guided_begin_tactics (tactics = 0: no solver stage) and flags.
 *     flags = 0: exactly epa_guided_begin_tactics, the same launches and the same bytes.
 *   epa_guided_proof, at any time: value int8 [k], the root's proven value for its mover; q int8 [k][A], per legal
 *     root action the proven value of its child for the root's mover; EPA_GUIDED_UNPROVEN for unproven, no child,
 *     illegal, a root that is over, and everywhere for a session without the flag.
 *   EPA_ERR_INVALID, before any launch, beside the refusals of epa_guided_begin_tactics: a flags bit other than
 *     EPA_GUIDED_PROVE.
 * The _device forms take device pointers and only enqueue. */
#define EPA_GUIDED_PROVE 1
#define EPA_GUIDED_UNPROVEN (-128)
int epa_guided_begin_prove(epa_pool* pool, const int32_t* env_ids, int32_t k, int32_t simulations, int32_t nodes,
                           int32_t width, float c_puct, int32_t tactics, int64_t tactics_nodes, int32_t flags,
                           uint8_t* obs, uint8_t* mask, uint8_t* status);
int epa_guided_begin_prove_device(epa_pool* pool, const int32_t* env_ids, int32_t k, int32_t simulations,
                                  int32_t nodes, int32_t width, float c_puct, int32_t tactics, int64_t tactics_nodes,
                                  int32_t flags, void* device_obs, void* device_mask, void* device_status);
int epa_guided_proof(epa_pool* pool, int8_t* value, int8_t* q);
int epa_guided_proof_device(epa_pool* pool, void* device_value, void* device_q);

/* Gumbel search (no reference analogue; the four PGX board games): the guided-search session above with a second
 * selection policy -- Gumbel top-m sampling without replacement at the root, sequential halving of the simulations
 * over those m actions, a deterministic rule inside the tree, and the improved policy softmax(logits + sigma(completed
 * Q)) as the training target (Danihelka et al., "Policy improvement by planning with Gumbel", ICLR 2022).  It needs
 * far fewer simulations per move than PUCT.  The session, its statuses, the emitted leaves, expansion, terminal
 * leaves, the backup and the session rules are those of epa_guided_begin; what differs (csrc/pgx_gumbel.hip.h is the
 * authority; nothing is pinned to another implementation's floating point):
 *   begin(ids, S, m, c_visit, c_scale, gumbel[k, A]):  m = the most root actions considered, 1 .. A (a larger one
 *     counts as A: a root considers min(m, its legal actions), so 16 serves every game);  c_visit, c_scale
 *     finite and >= 0 (the paper: 50 and 0.1);  gumbel: the caller's Gumbel(0, 1) noise per root action, float; a
 *     non-finite entry counts as 0; all zeros is the noise-free evaluation mode.  The library draws no random numbers.
 *   advance(logits[k, A], values[k]) -- call number t = 0 .. S:  logits are the policy's raw scores (any sign; a
 *     non-finite entry or one above 1e30 in magnitude counts as 0), values as for epa_guided_advance.  Entries of
 *     illegal actions are never read.  The host forms refuse such rows with EPA_ERR_INVALID before any launch.
 *   A node also holds raw (the caller's value of the node, as seat 0's; (float) term0 for a finished node) and per
 *   action logit[a] and p[a] = the softmax of the node's logits over its legal actions, floored at FLT_MIN.
 *   Per node, over its legal actions, sign as above, all float, in this order, nothing fused:
 *     N = sum of v[a];  vmax = max of v[a];  sraw = sign * raw;  q(a) = (sign * w0[a]) / v[a]   (where v[a] > 0)
 *     v_mix = N == 0 ? sraw : (sraw + N * (SUM_{v>0}(p[a] * q(a)) / SUM_{v>0}(p[a]))) / (1 + N)
 *     cq(a) = v[a] > 0 ? q(a) : v_mix;  scale = min((c_visit + vmax) * c_scale, 1e30)
 *     sg(a) = (scale * (cq(a) - min cq)) / max(max cq - min cq, 1e-8)
 *     pi'(a) = softmax over the legal actions of logit[a] + sg(a)
 *   interior pick:  argmax of pi'(a) - v[a] / (1 + N); ties: the lowest a
 *   root pick at simulation t = N(root):  m_eff = min(m, legal root actions);  cv = the t-th entry of the sequence
 *     of considered visits of sequential halving for (m_eff, S);  argmax over the legal a with v[a] == cv of
 *     (gumbel[a] + (logit[a] - max legal logit)) + sg(a); ties: the lowest a.  No such action ends the root with
 *     status 2 and sets the pool's error word.
 *   The exponential is the header's own (float + - * only, the argument clamped to [-87, 0]) and every float sum
 *   over actions has one stated order, so the kernels and the header's host build agree bit for bit.
 * epa_gumbel_result is valid any time after begin and complete after S + 1 advances:
 *   visits, values   as epa_guided_result
 *   action  [k]    int32   the root pick with cv = vmax: the recommended move; -1 for a root that was over
 *   weights [k, A] float   pi' of the root: 0 on illegal actions, sums to 1; the training target (zeros: root over)
 * A pool's one session has one policy.  epa_gumbel_begin replaces an open session of either policy, as
 * epa_guided_begin does; epa_guided_end ends a session of either policy.  EPA_ERR_INVALID: epa_guided_advance or
 * epa_guided_result on a Gumbel session, epa_gumbel_advance or epa_gumbel_result on a PUCT session; and the checks of
 * the guided calls, with m below 1 and c_visit / c_scale negative or not finite beside them.  Every family
 * without guided search fails with EPA_ERR_RUNTIME "gumbel search not implemented for this environment".
 * The _device forms take device pointers (float and int32 arrays 4-byte aligned) and only enqueue. */
int epa_gumbel_begin(epa_pool* pool, const int32_t* env_ids, int32_t k, int32_t simulations, int32_t max_considered,
                     float c_visit, float c_scale, const float* gumbel, uint8_t* obs, uint8_t* mask, uint8_t* status);
int epa_gumbel_begin_device(epa_pool* pool, const int32_t* env_ids, int32_t k, int32_t simulations,
                            int32_t max_considered, float c_visit, float c_scale, const void* device_gumbel,
                            void* device_obs, void* device_mask, void* device_status);
int epa_gumbel_advance(epa_pool* pool, const float* logits, const float* values, int32_t k, uint8_t* obs,
                       uint8_t* mask, uint8_t* status);
int epa_gumbel_advance_device(epa_pool* pool, const void* device_logits, const void* device_values, int32_t k,
                              void* device_obs, void* device_mask, void* device_status);
int epa_gumbel_result(epa_pool* pool, int32_t* visits, float* values, int32_t* action, float* weights);
int epa_gumbel_result_device(epa_pool* pool, void* device_visits, void* device_values, void* device_action,
                             void* device_weights);

/* Gumbel search, a halving level per launch (csrc/pgx_gumbel.hip.h "A level per launch" is the authority): a BATCH
 * session of batch B, 1 .. EPA_GUMBEL_MAX_BATCH, keeps B slots per root -- each a pending leaf, a status and a path --
 * and one advance answers every pending slot and then makes up to B simulations of the root's current LEVEL of
 * sequential halving (the run of simulations with the same considered visit count).  They go through different root
 * actions, so their descents live in disjoint subtrees: no virtual loss, no collision, nothing dropped.  S = 32 with
 * m = 16 and B = 16 costs 5 model calls of k * B rows (levels of 16, 8, 4, 4) instead of 33 calls of k rows.
 *   The root rule is the batch session's own: a launch scores the root ONCE, on the tree as it stands after the
 *   answers -- t = N(root), cv as above, r = what is left of the level, b = min(B, r) -- and takes the b legal actions
 *   with v[a] == cv of the largest (gumbel[a] + (logit[a] - max legal logit)) + sg(a), ties the lowest a, in that
 *   order, for slots 0 .. b-1 (fewer if there are fewer; none ends the root as above).  Below the root each descent
 *   is the plain session's.  The plain session re-scores the root before every simulation, so with values that are
 *   not constant the two give different results; B = 1 is the plain session call for call, bit for bit.
 *   Through this interface a batch session is a session of k * B rows: obs, mask and status of begin and advance, and
 *   logits and values of advance, have k * B rows, row i * B + j for slot j of root i; `k` of epa_gumbel_advance is
 *   k * B.  The noise has one row per root, and epa_gumbel_result gives one row per root.
 *   A slot of status 2 has nothing pending and its rows are zeros.  A round is complete when all k * B statuses are 2:
 *   for a root of m_eff considered actions after 1 + the sum over its levels of ceil(level size / B) advances, at most
 *   S + 1; later advances up to call number S change nothing, and a call number above S is refused.  Each root keeps
 *   S + 1 nodes, as in the plain session.
 *   EPA_ERR_INVALID, before any launch, beside the refusals of epa_gumbel_begin: a batch outside 1 ..
 *     EPA_GUMBEL_MAX_BATCH; advance with a row count other than k * B.  The tree limit EPA_SEARCH_MAX_TREE_BYTES counts
 *     the batch root records (about 1 KiB per slot).  epa_guided_reroot refuses every Gumbel session.
 * The _device form takes device pointers and only enqueues. */
#define EPA_GUMBEL_MAX_BATCH 32
int epa_gumbel_begin_batch(epa_pool* pool, const int32_t* env_ids, int32_t k, int32_t simulations,
                           int32_t max_considered, int32_t batch, float c_visit, float c_scale, const float* gumbel,
                           uint8_t* obs, uint8_t* mask, uint8_t* status);
int epa_gumbel_begin_batch_device(epa_pool* pool, const int32_t* env_ids, int32_t k, int32_t simulations,
                                  int32_t max_considered, int32_t batch, float c_visit, float c_scale,
                                  const void* device_gumbel, void* device_obs, void* device_mask,
                                  void* device_status);

/* Built-in network (no reference analogue; the four PGX board games; csrc/pgx_net.hip.h is the authority): an
 * NNUE-style policy-value network in exact integer arithmetic, evaluated by one kernel on the int8 matrix cores, as
 * the evaluator of the guided and Gumbel sessions above.  Input: a leaf's obs, F = H W C bytes 0 / 1.  Layers: a trunk
 * of width D, L residual blocks, a head of A + 1 rows (policy, value); int8 weights -127 .. 127, int32 biases of at
 * most 2^30 in magnitude, rounding right shifts 0 .. 24, activations clamped to 0 .. 127.  Outputs, float32:
 * logit[a] = p[a] * scale_p, value = clamp(p[A] * scale_v, -1, 1).  A kernel, a host build and a numpy restatement of
 * the contract agree bit for bit.
 *   The blob: 32 bytes { uint32 magic "PGXN", int32 version = 1, F, A, D, L, float scale_p, scale_v }, then the 2 L + 2
 *   layers (trunk, the blocks' two each, head), each int8 [N][K] row-major padded with zeros to a multiple of 4 bytes,
 *   int32 bias [N], int32 shift (the head's is 0).  D a multiple of 32 in 32 .. 512, L 0 .. 8, F 1 .. 512, A 1 .. 127,
 *   scales finite in (0, 1e20].
 *   A net is created on a device and belongs to it, not to a pool: any pool of that device whose epa_guided_shape
 *   gives the same F and A can use it.  It owns one device allocation (the weights in the kernel's layout and the
 *   policy / value rows of its own evaluations, grown to the largest row count seen).  Calls that use one net must not
 *   overlap.
 *   The eval call (pool, net, rows, mode, obs [rows, F], mask [rows, A], status [rows]) -> policy float [rows, A],
 *   value float [rows]: one launch on the pool's stream.  mode EPA_NET_LOGITS: policy = the logits, written for every
 *   action.  mode EPA_NET_PRIORS: the softmax over the legal actions of mask (zero elsewhere), computed as the Gumbel
 *   kernels compute theirs.  A row whose status is not 0 gets a zero policy row and value 0.
 *   The run call (pool, net, advances, obs, mask, status, &made) works on the pool's open session of either policy (a
 *   PUCT session is fed priors, a Gumbel session logits): `advances` = n >= 1 enqueues n pairs of evaluation and
 *   advance without a host wait; 0 runs until the round is complete, at most simulations + 1 advances in all -- a plain
 *   session without a host wait, a wide or batch session with one read of a device word per advance.  obs, mask and
 *   status are in / out: the leaves of begin, of the last advance or of reroot go in, the last leaves come out.  The
 *   session's call counter moves as if the caller had made the advances; `made` (may be null) receives their number.
 *   EPA_ERR_INVALID: a blob that is no network (the message names the field), a device index out of range; a net of
 *   another device or of another F or A than the pool's; the run call without an open session or with `advances`
 *   outside 0 .. simulations + 1 less the advances made; rows < 1, an unknown mode, null arguments.
 *   Every family without guided search fails with EPA_ERR_RUNTIME "guided search not implemented for this
 *   environment".
 * The _device forms take device pointers (float arrays 4-byte aligned) and only enqueue on the pool's stream; the
 * run call's _device form with advances = 0 on a wide or batch session still waits once per advance. */
#define EPA_NET_LOGITS 0
#define EPA_NET_PRIORS 1
typedef struct epa_net epa_net;
int epa_net_create(int32_t device, const void* blob, size_t bytes, epa_net** out);
int epa_net_destroy(epa_net* net);
int epa_net_eval(epa_pool* pool, epa_net* net, int32_t rows, int32_t mode, const uint8_t* obs, const uint8_t* mask,
                 const uint8_t* status, float* policy, float* value);
int epa_net_eval_device(epa_pool* pool, epa_net* net, int32_t rows, int32_t mode, const void* device_obs,
                        const void* device_mask, const void* device_status, void* device_policy, void* device_value);
int epa_net_run(epa_pool* pool, epa_net* net, int32_t advances, uint8_t* obs, uint8_t* mask, uint8_t* status,
                int32_t* made);
int epa_net_run_device(epa_pool* pool, epa_net* net, int32_t advances, void* device_obs, void* device_mask,
                       void* device_status, int32_t* made);

/* Self-play recorder (no reference analogue; the four PGX board games; csrc/pgx_record.hip.h is the authority): a
 * pool's finished games as training samples on the device.  The recorder stages, per env, the positions and policy
 * targets of the game in progress; when the game ends it writes one sample per staged ply -- or one per ply and board
 * symmetry with EPA_RECORD_SYMMETRIES -- into seven arrays of `capacity` rows:
 *   obs uint8 [H, W, C] of the seat to move, mask uint8 [A], policy float32 [A], value float32 (the game's last
 *   reward for the seat that moved at the sample), ply int32 (the position's elapsed step), env_id int32 (global),
 *   sym uint8 (the symmetry's index, 0: the identity)
 * A pool has one recorder; its memory is one device allocation of its own, released by epa_record_end, by the next
 * epa_record_begin and by epa_destroy, and independent of a guided-search session, which may be open at the same time.
 *   epa_record_begin(capacity, max_plies, flags): max_plies = 0 means EPA_RECORD_DEFAULT_PLIES (no game of the four
 *     lasts longer than 122 plies).  The staging is num_envs x max_plies rows of {the 64-byte position, the elapsed
 *     step, the policy row}.
 *   epa_record_add(env_ids[k], policy[k][A]): BEFORE the step.  Row i is skipped if env env_ids[i] is over (also
 *     before its first reset).  If the env has more staged plies than elapsed steps they belong to an abandoned game
 *     (a forced reset, a restore) and are discarded: dropped_games += 1, dropped_plies += their number.  Then, if
 *     max_plies plies are staged, the ply is not staged (dropped_plies += 1); otherwise the position, its elapsed step
 *     and policy'[a] = (a is legal and policy[a] is finite) ? policy[a] : 0 are staged.  No normalisation.
 *   epa_record_finish(env_ids[k], reward[k][2], done[k]): AFTER the step, with what it returned.  Rows with done and
 *     staged plies are finished games of c_i = plies x nsym samples; off_i is the exclusive prefix sum of c_i in row
 *     order and base the sample count.  Game i is written at base + off_i iff base + off_i + c_i <= capacity, otherwise
 *     dropped whole (dropped_games += 1, dropped_plies += its plies).  The count becomes base + the sum of c_i of the
 *     written games.  Either way the env's staging is empty afterwards; rows with done = 0 are untouched.  Within a game
 *     the samples are ordered by ply, then by symmetry.  The result depends on the arguments and the positions only.
 *   epa_record_counters(out[5]): the sample count, then samples and games written, dropped_games and dropped_plies
 *     since begin.
 *   epa_record_drain(rows, ...): copies the `rows` samples to the host and sets the count to 0; `rows` must equal the
 *     sample count (epa_record_counters), which *count receives in any case.
 *   epa_record_view_device(arrays[7], count): the seven device arrays over the full capacity, in the order above, and
 *     the device int32 count; rows at and above the count are undefined.  epa_record_clear sets the count to 0.
 *   epa_record_discard(env_ids[k]): forgets the staged plies of the listed envs (env_ids = NULL: of every env).
 *   epa_record_shape(out[5]): H, W, C, A and nsym of the open recorder.
 * Symmetries (sample j: obs'[s_j(cell)] = obs[cell], mask'[s_j(a)] = mask[a], policy'[s_j(a)] = policy[a]):
 *   TicTacToe, Othello: the dihedral group, nsym 8 -- j >= 4: first (r, c) -> (c, r); then j & 3 times
 *   (r, c) -> (c, n - 1 - r); Othello's pass is fixed.  ConnectFour: nsym 2, (r, c) -> (r, 6 - c).  Hex: nsym 2,
 *   (x, y) -> (10 - x, 10 - y); the swap action is fixed.
 * The host forms move the call's rows through a pinned block and synchronise once (drain: twice); the _device forms
 * take device pointers for the rows (4-byte aligned; env_ids stay host memory) and only enqueue on the pool's stream.
 * Both see the state every send issued before them has left.
 * Errors:
 *   EPA_ERR_INVALID: capacity < 1, max_plies outside 0 .. EPA_RECORD_MAX_PLIES, unknown flags, staging and samples
 *     above EPA_RECORD_MAX_BYTES; a call without a recorder; k <= 0, more than num_envs ids, an id outside the pool or
 *     listed twice; drain with rows other than the count.
 *   Every other family fails with EPA_ERR_RUNTIME "recorder not implemented for this environment". */
#define EPA_RECORD_SYMMETRIES 1u
#define EPA_RECORD_MAX_PLIES 256
#define EPA_RECORD_DEFAULT_PLIES 128
#define EPA_RECORD_MAX_BYTES 2147483648ull
int epa_record_begin(epa_pool* pool, int32_t capacity, int32_t max_plies, uint32_t flags);
int epa_record_shape(epa_pool* pool, int32_t* out);
int epa_record_add(epa_pool* pool, const int32_t* env_ids, int32_t k, const float* policy);
int epa_record_add_device(epa_pool* pool, const int32_t* env_ids, int32_t k, const void* device_policy);
int epa_record_finish(epa_pool* pool, const int32_t* env_ids, int32_t k, const float* reward, const uint8_t* done);
int epa_record_finish_device(epa_pool* pool, const int32_t* env_ids, int32_t k, const void* device_reward,
                             const void* device_done);
int epa_record_drain(epa_pool* pool, int32_t rows, uint8_t* obs, uint8_t* mask, float* policy, float* value,
                     int32_t* ply, int32_t* env_id, uint8_t* sym, int32_t* count);
int epa_record_view_device(epa_pool* pool, void** arrays, void** count);
int epa_record_clear(epa_pool* pool);
int epa_record_discard(epa_pool* pool, const int32_t* env_ids, int32_t k);
int epa_record_counters(epa_pool* pool, int64_t* out);
int epa_record_end(epa_pool* pool);

/* Rollout collector (csrc/rollout.hip.h is the contract; DESIGN.md section 2 "Rollout collector"): an on-policy
 * trajectory buffer in device memory that the pool's own step fills, with episode statistics, GAE and observation
 * moments.  For pools with one row per env and a device step in sync mode: the PGX games and Atari return
 * EPA_ERR_RUNTIME "rollout not implemented for this environment", an async pool EPA_ERR_INVALID.  N = num_envs,
 * T = horizon.  The buffers, rows in env id order: one [T+1][N][row] array per state key whose name starts with "obs",
 * action [T][N][row], reward float32 [T][N], term, trunc, mask uint8 [T][N].
 *   epa_rollout_begin(horizon >= 1, episodes >= 0, flags): one collector per pool, a new one replaces it; the buffers
 *     must stay within EPA_ROLLOUT_MAX_BYTES.  EPA_ROLLOUT_MOMENTS: keep count, sum and sum of squares (float64) per
 *     component of the float obs keys.  While a collector is open epa_reset is refused (EPA_ERR_INVALID).
 *   epa_rollout_shape(out[8]): T, N, episodes, t (steps collected), obs keys, moment components, the step counter, flags.
 *   epa_rollout_reset(device, ptrs, n_ptrs, cap_rows, k_out): resets every env, stores the observations into slot 0,
 *     clears the carried done flags and the episode accumulators, t = 0; then device == 0: what epa_recv does with
 *     ptrs (host arrays of cap_rows rows), else what epa_recv_device does (ptrs receive device pointers).
 *   epa_rollout_step(action, out_ptrs, ...) / epa_rollout_step_device(d_action, wait_event, d_out_ptrs, ...): one step of
 *     every env in id order -- epa_step_device, then the collector's kernels on the pool's stream -- and what epa_recv /
 *     epa_recv_device returns.  EPA_ERR_INVALID before the first reset, with rows pending, and when t == T.
 *   epa_rollout_view_device(arrays[n]): the device arrays, obs keys first, then action, reward, term, trunc, mask.
 *   epa_rollout_batch(out_ptrs[n]): the same arrays copied whole to the host (a null pointer skips its array).
 *   epa_rollout_gae(values [T+1][N], gamma, lam, adv, ret [T][N]) / _device: needs t == T; gamma, lam in [0, 1].
 *   epa_rollout_episodes(rows, env_id, step, ret, length, count): the finished episodes (global env id, the step counter
 *     of the step that ended it, the float64 return, the length) to the host, and the count back to 0; `rows` must equal
 *     the count (epa_rollout_counters), which *count receives in any case.
 *   epa_rollout_episodes_view_device(arrays[4], count): the four device arrays over the capacity and the device int32
 *     count, read-only.
 *   epa_rollout_moments(out, d_out): [3][components] float64 -- count, sum, sumsq -- to the host (out, may be NULL) and
 *     the device address of the same (d_out, may be NULL).
 *   epa_rollout_next(): obs slot t becomes slot 0, t = 0; everything else is kept.
 *   epa_rollout_counters(out[6]): episode rows, episodes finished and dropped since begin, the step counter, t, and
 *     whether a reset has run.
 *   epa_rollout_end(): releases the collector. */
#define EPA_ROLLOUT_MOMENTS 1u
#define EPA_ROLLOUT_MAX_BYTES 2147483648ull
int epa_rollout_begin(epa_pool* pool, int32_t horizon, int32_t episodes, uint32_t flags);
int epa_rollout_shape(epa_pool* pool, int64_t* out);
int epa_rollout_reset(epa_pool* pool, int32_t device, void** ptrs, int32_t n_ptrs, int32_t cap_rows, int32_t* k_out);
int epa_rollout_step(epa_pool* pool, const void* action, void* const* out_ptrs, int32_t n_ptrs, int32_t cap_rows,
                     int32_t* k_out);
int epa_rollout_step_device(epa_pool* pool, const void* d_action, void* wait_event, void** d_out_ptrs, int32_t n_ptrs,
                            int32_t* k_out);
int epa_rollout_view_device(epa_pool* pool, void** arrays, int32_t n);
int epa_rollout_batch(epa_pool* pool, void* const* out_ptrs, int32_t n);
int epa_rollout_gae(epa_pool* pool, const float* values, float gamma, float lam, float* adv, float* ret);
int epa_rollout_gae_device(epa_pool* pool, const void* d_values, float gamma, float lam, void* d_adv, void* d_ret);
int epa_rollout_episodes(epa_pool* pool, int32_t rows, int32_t* env_id, int64_t* step, double* ret, int32_t* length,
                         int32_t* count);
int epa_rollout_episodes_view_device(epa_pool* pool, void** arrays, void** count);
int epa_rollout_moments(epa_pool* pool, double* out, void** d_out);
int epa_rollout_next(epa_pool* pool);
int epa_rollout_counters(epa_pool* pool, int64_t* out);
int epa_rollout_end(epa_pool* pool);

/* Rollout actor (csrc/actor.hip.h is the contract; DESIGN.md section 2 "Rollout actor and collect"): a built-in int8
 * actor-critic attached to the pool's open collector, so that a whole horizon is played from C++ with nothing between
 * the launches.  The blob: magic "EPAA", version 1, F, H, D, L, kind, scale_p, scale_v, lo[F], scale[F] float64,
 * sigma[H] float32 (EPA_ACTOR_BOX only), then the layer section of a network blob (epa_net_create).
 *   epa_actor_begin(blob, bytes, seed, flags, actions, low, high): checks the blob and compares it with the pool -- F =
 *     the components of the collector's obs keys (at most 512), kind and H with the action row, `actions` (the number
 *     of discrete actions, or the Box dimension) with H; low / high: the Box bounds, float64 [H] (NULL for a discrete
 *     space).  EPA_ERR_INVALID on a mismatch and without an open collector.  It adds logp float32 [T][N] and value
 *     float32 [T+1][N] to the collector, counted in EPA_ROLLOUT_MAX_BYTES.  EPA_ACTOR_DETERMINISTIC: the mode of the
 *     policy instead of a sample.  One actor per collector; a new one replaces it, and it goes with the collector.
 *   epa_actor_shape(out[4]): F, H, kind, flags.
 *   epa_rollout_collect(steps) / _device: `steps` steps (0: the rest of the horizon) of features of slot t, the net, the
 *     sample and what epa_rollout_step_device enqueues, then the value of slot t; the host form waits for the stream
 *     once, the device form only enqueues.  EPA_ERR_INVALID before the first reset, with rows pending, when t == T and
 *     when t + steps > T.
 *   epa_actor_eval(env_ids, k, step, obs[n_obs], action, logp, value) / _device: the actor on k rows of caller
 *     observations (one array per obs key, rows of the key's shape) for the listed global env ids at step counter
 *     `step`: the action rows of the pool's action dtype, logp and value float32 [k].  Nothing of the pool changes.
 *   epa_actor_view_device(logp, value): the device arrays.  epa_actor_batch(logp, value): copied whole to the host
 *     (NULL skips one).  epa_rollout_gae with values == NULL takes the stored values.
 *   epa_actor_end(): releases the actor. */
#define EPA_ACTOR_DETERMINISTIC 1u
#define EPA_ACTOR_DISCRETE 0
#define EPA_ACTOR_BOX 1
int epa_actor_begin(epa_pool* pool, const void* blob, size_t bytes, uint64_t seed, uint32_t flags, int32_t actions,
                    const double* low, const double* high);
int epa_actor_shape(epa_pool* pool, int64_t* out);
int epa_actor_end(epa_pool* pool);
int epa_actor_eval(epa_pool* pool, const int32_t* env_ids, int32_t k, int64_t step, const void* const* obs,
                   int32_t n_obs, void* action, float* logp, float* value);
int epa_actor_eval_device(epa_pool* pool, const void* d_env_ids, int32_t k, int64_t step, const void* const* d_obs,
                          int32_t n_obs, void* d_action, void* d_logp, void* d_value);
int epa_actor_view_device(epa_pool* pool, void** logp, void** value);
int epa_actor_batch(epa_pool* pool, float* logp, float* value);
int epa_rollout_collect(epa_pool* pool, int32_t steps);
int epa_rollout_collect_device(epa_pool* pool, int32_t steps);

/* Self-play driver (no reference analogue; the four PGX board games; csrc/pgx_selfplay.hip.h is the authority): one
 * call plays `plies` plies of EVERY env of a pool against itself with the built-in network as the evaluator, with
 * auto-resets, and -- with `record` -- the finished games land in the pool's open recorder.  Everything is enqueued
 * through the device forms above; between two plies nothing leaves the device.
 *   One ply, over all envs of the pool in id order: the root noise (Gumbel sessions; PgxSelfplayNoise), the begin of a
 *   session of `policy` (its leaf arrays live in the driver's block), the whole round with the net (epa_net_run_device,
 *   advances = 0), the result, the move (PgxSelfplayMove: the action row and the policy target rows), epa_record_add,
 *   the step (epa_send_device + epa_recv_device, whose batch is pending at once), epa_record_finish on the result
 *   block's reward and done, the tally (PgxSelfplayTally).  An env that is over gets action 0, which resets it, so the
 *   games follow each other without the host.
 *   Contract (csrc/pgx_selfplay.hip.h).  The driver counts its plies: t = 0 at begin, + 1 per ply, across run calls.
 *   key(e, t) = SM(seed ^ SM((uint64(global env id e) << 32) | uint32(t))), SM = splitmix64 as in epa_playout.  Noise:
 *   u = ((float)(SM(key + a) >> 41) + 0.5) * 2^-23, g[a] = -GumbelLog(-GumbelLog(u)), GumbelLog a float32 logarithm of
 *   the library's own (bit-identical on host and device); noise = 0: zero rows.  Gumbel move: the result's action, 0 for
 *   -1; target = the result's weights.  PUCT move: V = the sum of the root's visits; V = 0 or a root that was over:
 *   action 0 and a zero target; otherwise target[a] = visits[a] / V, and the action is, while the env's elapsed step is
 *   below sample_plies, the lowest a whose inclusive prefix sum of visits exceeds ((SM(key + 0x100) >> 32) * V) >> 32,
 *   afterwards the most visited action (the lowest on ties).  Statistics: games, wins of seat 0 (its last reward > 0),
 *   wins of seat 1, draws (both 0), plies (the sum of the finished games' elapsed steps).
 *   epa_selfplay_begin(pool, net, options): opens the driver (a pool has one; a new one replaces it).  Its memory is
 *     one device allocation of its own, released by epa_selfplay_end, the next begin and epa_destroy; it coexists with
 *     the session and the recorder.  The options are those of epa_gumbel_begin_batch (policy EPA_SELFPLAY_GUMBEL:
 *     simulations, max_considered, c_visit, c_scale, batch) or of epa_guided_begin_prove (EPA_SELFPLAY_PUCT:
 *     simulations, c_puct, width, tactics, tactics_nodes, prove, and sample_plies), checked as those check them; every
 *     field of the other policy must be 0 -- a Gumbel driver: c_puct, width, tactics, prove, tactics_nodes,
 *     sample_plies; a PUCT driver: max_considered, batch, c_visit, c_scale, noise -- and is refused otherwise.
 *   epa_selfplay_run(pool, plies): plays and waits for the device; epa_selfplay_run_device only enqueues on the pool's
 *     stream (a batch or width session still reads one device word per advance, as epa_net_run does).  The driver uses
 *     the pool's guided-search session: an open one is replaced, and the last ply's session stays open.
 *   epa_selfplay_stats(out[6]): games, wins0, wins1, draws, plies, t since begin -- the one host wait.
 *   A run call that fails partway (a device error, a recorder closed by another thread) has enqueued its earlier
 *   plies and part of one more, whose recorder add may lack its finish, and t does not count the partial ply: close
 *   the driver (epa_selfplay_end) and discard the recorder's staging (epa_record_discard) after such an error.
 * Errors (before any launch):
 *   EPA_ERR_RUNTIME "guided search not implemented for this environment" / "recorder not implemented ..." for the other
 *     families.
 *   EPA_ERR_INVALID: a net of another device or of other F / A; rows pending in the pool's result queue; async mode
 *     (batch_size != num_envs); record without an open recorder; plies < 1; an unknown policy; option values the
 *     session's begin refuses; options of the other policy; a call without a driver. */
#define EPA_SELFPLAY_GUMBEL 0
#define EPA_SELFPLAY_PUCT 1
typedef struct epa_selfplay_options {
  int32_t policy;
  int32_t simulations;
  int32_t max_considered; /* Gumbel */
  int32_t batch;          /* Gumbel; 0: a plain session */
  float c_visit;          /* Gumbel */
  float c_scale;          /* Gumbel */
  float c_puct;           /* PUCT */
  int32_t width;          /* PUCT; 0: a plain session */
  int32_t tactics;        /* PUCT */
  int32_t prove;          /* PUCT */
  int64_t tactics_nodes;  /* PUCT */
  uint64_t seed;
  int32_t noise;          /* Gumbel: 0 zero rows */
  int32_t sample_plies;   /* PUCT */
  int32_t record;         /* 1: add / finish on the pool's open recorder */
  int32_t reserved;       /* 0 */
} epa_selfplay_options;
int epa_selfplay_begin(epa_pool* pool, epa_net* net, const epa_selfplay_options* options);
int epa_selfplay_run(epa_pool* pool, int32_t plies);
int epa_selfplay_run_device(epa_pool* pool, int32_t plies);
int epa_selfplay_stats(epa_pool* pool, int64_t* out);
int epa_selfplay_end(epa_pool* pool);

/* PUCT exploration of the driver and the arena (csrc/pgx_dirichlet.hip.h is the authority): Dirichlet root noise and a
 * move temperature, the two pieces of standard AlphaZero self-play the options above lack.
 *   dirichlet_alpha > 0: every ply draws eta ~ Dir(alpha) over the legal root actions of every env -- one Gamma(alpha)
 *     variate per (env, action) by a boosted Marsaglia-Tsang sampler on the counter-based uniforms of key(e, t), at the
 *     indices 0x200 + ((a * 16 + j) * 4 + c), normalised by a float32 sum in one fixed order -- and mixes it into the
 *     priors of the roots, p' = (1 - eps) p + eps eta, between the round's first evaluation and its first advance
 *     (PgxSelfplayDirichlet; an arena: after the pair evaluation of the roots), so the tree stores the mixed priors.  A
 *     root that is over is left alone.  alpha > 0 with eps == 0 draws and mixes nothing in.  alpha == 0: no noise.
 *   temperature T != 1: while a game's elapsed step < sample_plies the move is sampled from visits^(1/T), as integers
 *     q[a] = (uint32)(exp_(log_(visits[a] / max visits) / T) * 2^20) through the pick of the plain rule; the policy
 *     target stays visits / SUM visits.  T == 1 is the plain rule, byte for byte.
 *   epa_selfplay_begin_ex(pool, net_a, net_b, options, extra): epa_selfplay_begin (net_b NULL) or epa_arena_begin with
 *     `extra`; those two behave as extra = {0, 0, 1, 0}.
 *   epa_selfplay_noise(pool, out): the host copy of the last ply's noise rows, float32 [num_envs][A] -- eta of a PUCT
 *     driver (zeros without alpha, and before the first ply), the Gumbel rows of a Gumbel driver.  Waits for the device.
 * Errors (before any launch), EPA_ERR_INVALID: dirichlet_alpha not finite or outside 0 .. 100; dirichlet_eps outside
 *   0 .. 1; temperature outside 0.05 .. 20; reserved != 0; a Gumbel driver with any of the three other than 0 / 0 / 1;
 *   epa_selfplay_noise without a driver. */
typedef struct epa_selfplay_extra {
  float dirichlet_alpha;
  float dirichlet_eps;
  float temperature;
  int32_t reserved; /* 0 */
} epa_selfplay_extra;
int epa_selfplay_begin_ex(epa_pool* pool, epa_net* net_a, epa_net* net_b /* NULL: self-play */,
                          const epa_selfplay_options* options, const epa_selfplay_extra* extra);
int epa_selfplay_noise(epa_pool* pool, float* out);

/* Arena (no reference analogue; the four PGX board games; csrc/pgx_arena.hip.h is the authority): two networks play
 * each other in one pool, as a mode of the pool's one self-play driver.
 *   Which net moves: net (m ^ e) & 1 for seat m of the env with GLOBAL id e, 0 = net_a, 1 = net_b: net_a holds seat 0
 *   of the even envs and seat 1 of the odd ones, and the reset coin decides which seat moves first.  A ply's search
 *   tree is evaluated by its root mover's net throughout.
 *   epa_net_eval_pair(pool, net_a, net_b, rows, mode, obs, mask, status, side, policy, value): epa_net_eval with one
 *     side byte per row, 0 or 1: row r gets exactly the policy and value epa_net_eval of that net gives it.  The rows
 *     are grouped by net on the device (a stable partition, no atomics) and evaluated in one launch.  rows <= 2^20.
 *   epa_arena_begin(pool, net_a, net_b, options): epa_selfplay_begin with a second net; every rule, option and refusal
 *     of it applies to both nets, which agree in F and A with the pool (D and L may differ) and lie on its device.
 *     epa_selfplay_run, epa_selfplay_run_device and epa_selfplay_end drive and close an arena as they do a driver, and
 *     epa_selfplay_stats returns its six values.  A ply is the driver's with two changes: after the session's begin the
 *     side bytes of the leaf rows are written (PgxArenaSides) and grouped (PgxNetPlan), and the round runs with the
 *     pair evaluation.  Noise, move, recorder, step and the key are unchanged.
 *   epa_arena_stats(out[8]): games, wins0, wins1, draws, plies, wins_a (finished games whose last reward of net_a's
 *     seat, e & 1, is > 0), wins_b (of seat 1 - (e & 1)), t.  EPA_ERR_INVALID on a driver that is no arena.
 * Errors (before any launch): epa_selfplay_begin's and epa_net_eval's; the host form of epa_net_eval_pair refuses a side
 *   byte other than 0 or 1 (the device form reads any non-zero byte as 1); rows outside 1 .. 2^20. */
int epa_net_eval_pair(epa_pool* pool, epa_net* net_a, epa_net* net_b, int32_t rows, int32_t mode, const uint8_t* obs,
                      const uint8_t* mask, const uint8_t* status, const uint8_t* side, float* policy, float* value);
int epa_net_eval_pair_device(epa_pool* pool, epa_net* net_a, epa_net* net_b, int32_t rows, int32_t mode,
                             const void* device_obs, const void* device_mask, const void* device_status,
                             const void* device_side, void* device_policy, void* device_value);
int epa_arena_begin(epa_pool* pool, epa_net* net_a, epa_net* net_b, const epa_selfplay_options* options);
int epa_arena_stats(epa_pool* pool, int64_t* out);

/* ---- Atari post-process (K4): max-pool of the last two ALE frames, resize
 *      to 84x84, push into the frame stack (replaces AtariEnv::PushStack,
 *      envpool/atari/atari_env.h:308-346 + envpool/utils/image_process.h:27-36).
 *      use_inter_area: the config key `use_inter_area_resize` (atari_env.h:61):
 *      1 = cv::INTER_AREA (default), 0 = cv::INTER_LINEAR (what the reference's
 *      benchmark/test_envpool.py:92 selects). */
typedef struct epa_atari_post epa_atari_post;
int epa_atari_post_create(int32_t num_envs, int32_t stack_num, int32_t in_h,
                          int32_t in_w, int32_t out_h, int32_t out_w,
                          int32_t use_inter_area, int32_t device,
                          epa_atari_post** out);
/* As above, plus the colour handling of atari_env.h:189-194 / 213-219 / 320-335:
 *   palette != NULL: the frames handed to push are ALE palette INDICES (the emulator's
 *     screen, 1 byte per pixel) and `palette` is the table behind applyPaletteGrayscale
 *     ([256], gray_scale = 1) or applyPaletteRGB ([3][256] planar, gray_scale = 0); it is
 *     applied on the device, per frame before the max-pool.
 *   gray_scale = 0 (needs the palette): a stacked frame is three planes [3, out_h, out_w]
 *     (the transpose of atari_env.h:320-335), observations are
 *     [k, stack_num * 3, out_h, out_w].
 * Refused with EPA_ERR_INVALID (the message names the reason):
 *   - stack_num < 1, an output larger than the raw frame, in_h * in_w > 60000;
 *   - in_h * in_w not a multiple of 16 (the kernel reads the raw frames with aligned 16-byte
 *     loads; Atari's 210 x 160 is);
 *   - ceil16(in_h * in_w) + 28 * (out_h + out_w) + 256 * planes > 65536: one block stages the
 *     raw frame, both tap tables and the palette in LDS (240 x 244 -> 100 x 100 RGB, 64928
 *     bytes, is accepted; 240 x 248 is not);
 *   - INTER_AREA with more than 6 taps on an axis (scale > ~5) or with integer scale factors,
 *     INTER_LINEAR with an exact 2 x 2 reduction (OpenCV fast paths that are not restated). */
int epa_atari_post_create_ex(int32_t num_envs, int32_t stack_num, int32_t in_h,
                             int32_t in_w, int32_t out_h, int32_t out_w,
                             int32_t use_inter_area, int32_t gray_scale,
                             const uint8_t* palette, int32_t device,
                             epa_atari_post** out);
int epa_atari_post_destroy(epa_atari_post* p);
/* frames: [k, 2, in_h, in_w] u8 (the two max-pool buffers, host memory);
 * reset_mask[k] u8 (NULL = all 0), per-row flags of AtariEnv::PushStack (atari_env.h:308-346):
 *   0  max-pool the two frames, push                       (Step, frame_skip loop completed)
 *   1  frame 0 only, replicated into every stack slot      (Reset with push_all)
 *   2  frame 0 only, pushed like a step                    (Reset of an episodic-life env,
 *                                                           frame_skip = 1, early game over)
 *   4  no new screen: push the newest stacked frame again  (game over before a capture)
 * obs_out: [k, stack_num * (gray_scale ? 1 : 3), out_h, out_w] u8 host. */
int epa_atari_post_push(epa_atari_post* p, const int32_t* env_id, int32_t k,
                        const uint8_t* frames, const uint8_t* reset_mask,
                        uint8_t* obs_out);
/* device-resident variant: all pointers are device pointers (d_frames and d_obs_out
 * 16-byte aligned; d_env_id NULL = rows 0..k-1), the launch goes to
 * epa_atari_post_stream() and shares the frame-stack ring with epa_atari_post_push. */
int epa_atari_post_push_device(epa_atari_post* p, const int32_t* d_env_id,
                               int32_t k, const uint8_t* d_frames,
                               const uint8_t* d_reset_mask, uint8_t* d_obs_out);
void* epa_atari_post_stream(epa_atari_post* p);

/* ---- Atari end to end --------------------------------------------------- *
 * AtariEnvPool = AsyncEnvPool<AtariEnv> (envpool/atari/atari_env.h:348) as an epa_pool: the
 * emulator runs on host worker threads behind the plugin table of
 * include/envpool_amd_emulator.h, palette + max-pool + resize + frame stack run as one HIP
 * kernel per batch.  The pool is driven with the generic epa_send / epa_recv / epa_recv_block
 * / epa_reset / epa_destroy (the device-resident entry points raise: the emulator is on the
 * host).  Numeric config keys of AtariEnvFns::DefaultConfig (atari_env.h:52-63) travel in
 * base.param_*: stack_num frame_skip noop_max zero_discount_on_life_loss episodic_life
 * reward_clip use_fire_reset img_height img_width mode difficulty full_action_space
 * repeat_action_probability use_inter_area_resize gray_scale, plus num_threads. */
typedef struct epa_atari_config {
  epa_config base;
  const char* rom_path;     /* GetRomPath(base_path, task), atari_env.h:43-48 */
  const char* emulator_lib; /* emulator plugin, see envpool_amd_emulator.h */
} epa_atari_config;
int epa_atari_create(const epa_atari_config* cfg, epa_pool** out);
/* size of the action set (AtariEnvFns::ActionSpec loads the ROM for it, atari_env.h:76-90) */
int epa_atari_num_actions(const epa_atari_config* cfg, int32_t* n);
/* state / action keys of an existing pool (same order and meaning as epa_describe_*) */
int epa_pool_state_keys(epa_pool* pool, epa_key_info* keys, int cap, int* n);
int epa_pool_action_keys(epa_pool* pool, epa_key_info* keys, int cap, int* n);

/* ---- misc -------------------------------------------------------------- */
const char* epa_last_error(void);
const char* epa_version(void);
int epa_device_count(int32_t* n);
/* pinned host memory for zero-copy numpy hand-off (py_envpool.h:40-49) */
void* epa_host_alloc(size_t bytes);
void epa_host_free(void* p);

#ifdef __cplusplus
}
#endif
#endif /* ENVPOOL_AMD_H_ */
