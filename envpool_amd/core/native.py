"""ctypes binding of the C ABI declared in include/envpool_amd.h.

This is the reference-side stub a maintainer would write instead of
`PyEnvPool<AsyncEnvPool<Env>>` (envpool/core/py_envpool.h:206-288): the Python
adaptors keep calling `_send/_recv/_reset`, which land here.

There is NO CPU fallback: if the HIP library is missing, or no GPU is visible
when a pool is created, an exception is raised.
"""

from __future__ import annotations

import ctypes
import os
from typing import Any, Sequence

import numpy as np

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# ENVPOOL_AMD_LIB: another build of the same C ABI (the cross-check tests load lib/libenvpool_amd_alt.so, the
# product library plus the superseded Humanoid kernels: `make -C envpool_amd/csrc EPA_ALT_KERNELS=1`)
LIB_PATH = os.environ.get("ENVPOOL_AMD_LIB") or os.path.join(_PKG, "lib", "libenvpool_amd.so")

EPA_OK, EPA_ERR_INVALID, EPA_ERR_RUNTIME, EPA_ERR_DEVICE = 0, 1, 2, 3
EPA_SNAP_RNG = 1
SNAP_HEADER_BYTES = 64
EPA_PLAYOUT_COMMIT = 1
PLAYOUT_MAX_PLIES = 256
PLAYOUT_MAX_REPEATS = 4096
SEARCH_MAX_SIMULATIONS = 4096
GUIDED_MAX_NODES = 8192  # EPA_GUIDED_MAX_NODES: the largest node capacity of a guided-search root
GUIDED_MAX_WIDTH = 32    # EPA_GUIDED_MAX_WIDTH: the most slots (leaves per launch) of a wide guided-search root
GUIDED_MAX_TACTICS = 16  # EPA_GUIDED_MAX_TACTICS: the largest horizon of a guided search's exact leaf status
GUIDED_MAX_TACTICS_NODES = 1 << 20  # EPA_GUIDED_MAX_TACTICS_NODES: the largest node budget of one leaf's solve
GUIDED_TACTICS_NODES = 4096         # EPA_GUIDED_TACTICS_NODES: its default
GUIDED_PROVE = 1         # EPA_GUIDED_PROVE: the flag of a guided search with proven values
GUIDED_UNPROVEN = -128   # EPA_GUIDED_UNPROVEN: "no proven value" in guided_proof's arrays
GUMBEL_MAX_BATCH = 32    # EPA_GUMBEL_MAX_BATCH: the most slots (simulations per launch) of a batch Gumbel root
SEARCH_MAX_LEAF_PLAYOUTS = 64
RECORD_SYMMETRIES = 1    # EPA_RECORD_SYMMETRIES: the flag of a recorder that writes every board symmetry
RECORD_MAX_PLIES = 256   # EPA_RECORD_MAX_PLIES: the largest max_plies of a recorder (0: 128)
ROLLOUT_MOMENTS = 1      # EPA_ROLLOUT_MOMENTS: the flag of a rollout collector that keeps observation moments
ROLLOUT_MAX_BYTES = 1 << 31  # EPA_ROLLOUT_MAX_BYTES: the buffers of one rollout collector
ACTOR_DETERMINISTIC = 1  # EPA_ACTOR_DETERMINISTIC: a rollout actor that takes the mode of its policy
SOLVE_MAX_DEPTH = 128    # EPA_SOLVE_MAX_DEPTH: the plies of a solver's longest line
SOLVE_MAX_TABLE_BITS = 16  # EPA_SOLVE_MAX_TABLE_BITS: a lane's transposition table has at most 2^16 entries
SOLVE_ILLEGAL = -128     # q of an illegal action, and of every action of a row that is not solved
DTYPES = {0: np.int32, 1: np.float32, 2: np.float64, 3: np.bool_, 4: np.uint8, 5: np.int8}


class EpaConfig(ctypes.Structure):
    _fields_ = [
        ("num_envs", ctypes.c_int32),
        ("batch_size", ctypes.c_int32),
        ("seed", ctypes.c_int32),
        ("env_seed", ctypes.POINTER(ctypes.c_int32)),
        ("max_episode_steps", ctypes.c_int32),
        ("device", ctypes.c_int32),
        ("env_id_offset", ctypes.c_int32),
        ("n_params", ctypes.c_int32),
        ("param_keys", ctypes.POINTER(ctypes.c_char_p)),
        ("param_values", ctypes.POINTER(ctypes.c_double)),
    ]


class EpaAtariConfig(ctypes.Structure):
    _fields_ = [
        ("base", EpaConfig),
        ("rom_path", ctypes.c_char_p),
        ("emulator_lib", ctypes.c_char_p),
    ]


class EpaKeyInfo(ctypes.Structure):
    _fields_ = [
        ("name", ctypes.c_char_p),
        ("dtype", ctypes.c_int32),
        ("ndim", ctypes.c_int32),
        ("shape", ctypes.c_int32 * 4),
        ("row_elems", ctypes.c_int32),
        ("row_bytes", ctypes.c_int32),
    ]


_lib: ctypes.CDLL | None = None


def lib() -> ctypes.CDLL:
    """Load libenvpool_amd.so (built by `__graft_entry__.build()`)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"envpool_amd: HIP library not built ({LIB_PATH} missing). Run "
            "`python -c 'import __graft_entry__ as g; g.build()'` or "
            "`make -C envpool_amd/csrc`. There is no CPU fallback."
        )
    L = ctypes.CDLL(LIB_PATH)
    vp, i32, cp = ctypes.c_void_p, ctypes.c_int32, ctypes.c_char_p
    P = ctypes.POINTER
    sig = {
        "epa_num_families": (i32, []),
        "epa_family_name": (cp, [i32]),
        "epa_describe_state": (i32, [cp, P(EpaConfig), P(EpaKeyInfo), i32, P(i32)]),
        "epa_describe_action": (i32, [cp, P(EpaConfig), P(EpaKeyInfo), i32, P(i32)]),
        "epa_family_players": (i32, [cp, P(i32)]),
        "epa_describe_state_players": (i32, [cp, P(EpaConfig), P(i32), i32, P(i32)]),
        "epa_create": (i32, [cp, P(EpaConfig), P(vp)]),
        "epa_destroy": (i32, [vp]),
        "epa_send": (i32, [vp, vp, i32, vp]),
        "epa_send_into": (i32, [vp, vp, i32, vp, vp, ctypes.c_size_t]),
        "epa_reset": (i32, [vp, vp, i32]),
        "epa_recv": (i32, [vp, P(vp), i32, i32, P(i32)]),
        "epa_recv_layout": (i32, [vp, i32, P(ctypes.c_size_t), i32, P(ctypes.c_size_t)]),
        "epa_recv_block": (i32, [vp, vp, ctypes.c_size_t, P(ctypes.c_size_t), i32, P(i32)]),
        "epa_recv_into": (i32, [vp, P(vp), i32, i32, P(i32)]),
        "epa_pending_rows": (i32, [vp, P(i32)]),
        "epa_send_device": (i32, [vp, vp, i32, vp, vp]),
        "epa_wait_stream": (i32, [vp, vp]),
        "epa_consumer_wait": (i32, [vp, vp]),
        "epa_recv_device": (i32, [vp, P(vp), i32, P(i32)]),
        "epa_step_device": (i32, [vp, vp, i32, vp, vp, P(vp), i32, P(i32)]),
        "epa_stream": (vp, [vp]),
        "epa_synchronize": (i32, [vp]),
        "epa_set_timing": (i32, [vp, i32]),
        "epa_kernel_time_ms": (i32, [vp, P(ctypes.c_double), P(i32)]),
        "epa_state_dim": (i32, [vp, P(i32)]),
        "epa_get_state": (i32, [vp, vp, i32, vp]),
        "epa_set_state": (i32, [vp, vp, i32, vp]),
        "epa_render_size": (i32, [vp, i32, i32, P(i32), P(i32)]),
        "epa_render": (i32, [vp, vp, i32, i32, i32, i32, vp]),
        "epa_render_device": (i32, [vp, vp, i32, i32, i32, i32, vp]),
        "epa_snapshot_bytes": (i32, [vp, i32, ctypes.c_uint32, P(ctypes.c_size_t)]),
        "epa_snapshot": (i32, [vp, vp, i32, ctypes.c_uint32, vp, ctypes.c_size_t]),
        "epa_restore": (i32, [vp, vp, i32, vp, ctypes.c_size_t]),
        "epa_snapshot_device": (i32, [vp, vp, i32, ctypes.c_uint32, vp, vp]),
        "epa_restore_device": (i32, [vp, vp, i32, vp, vp]),
        "epa_fork": (i32, [vp, vp, vp, i32, ctypes.c_uint32]),
        "epa_playout": (i32, [vp, vp, i32, i32, i32, ctypes.c_uint64, ctypes.c_uint32, vp, vp, vp]),
        "epa_playout_device": (i32, [vp, vp, i32, i32, i32, ctypes.c_uint64, ctypes.c_uint32, vp, vp, vp]),
        "epa_search_actions": (i32, [vp, P(i32)]),
        "epa_search": (i32, [vp, vp, i32, i32, i32, ctypes.c_float, i32, ctypes.c_uint64, vp, vp, vp]),
        "epa_search_device": (i32, [vp, vp, i32, i32, i32, ctypes.c_float, i32, ctypes.c_uint64, vp, vp, vp]),
        "epa_solve": (i32, [vp, vp, i32, i32, ctypes.c_int64, vp, vp, vp, vp, vp]),
        "epa_solve_device": (i32, [vp, vp, i32, i32, ctypes.c_int64, vp, vp, vp, vp, vp]),
        "epa_solve_table": (i32, [vp, vp, i32, i32, ctypes.c_int64, i32, vp, vp, vp, vp, vp]),
        "epa_solve_table_device": (i32, [vp, vp, i32, i32, ctypes.c_int64, i32, vp, vp, vp, vp, vp]),
        "epa_guided_shape": (i32, [vp, P(i32)]),
        "epa_guided_begin": (i32, [vp, vp, i32, i32, ctypes.c_float, vp, vp, vp]),
        "epa_guided_begin_device": (i32, [vp, vp, i32, i32, ctypes.c_float, vp, vp, vp]),
        "epa_guided_advance": (i32, [vp, vp, vp, i32, vp, vp, vp]),
        "epa_guided_advance_device": (i32, [vp, vp, vp, i32, vp, vp, vp]),
        "epa_guided_result": (i32, [vp, vp, vp, vp]),
        "epa_guided_result_device": (i32, [vp, vp, vp, vp]),
        "epa_guided_end": (i32, [vp]),
        "epa_guided_begin_nodes": (i32, [vp, vp, i32, i32, i32, ctypes.c_float, vp, vp, vp]),
        "epa_guided_begin_nodes_device": (i32, [vp, vp, i32, i32, i32, ctypes.c_float, vp, vp, vp]),
        "epa_guided_reroot": (i32, [vp, vp, i32, i32, vp, vp, vp]),
        "epa_guided_reroot_device": (i32, [vp, vp, i32, i32, vp, vp, vp]),
        "epa_guided_begin_wide": (i32, [vp, vp, i32, i32, i32, i32, ctypes.c_float, vp, vp, vp]),
        "epa_guided_begin_wide_device": (i32, [vp, vp, i32, i32, i32, i32, ctypes.c_float, vp, vp, vp]),
        "epa_guided_begin_tactics": (i32, [vp, vp, i32, i32, i32, i32, ctypes.c_float, i32, ctypes.c_int64, vp, vp,
                                           vp]),
        "epa_guided_begin_tactics_device": (i32, [vp, vp, i32, i32, i32, i32, ctypes.c_float, i32, ctypes.c_int64, vp,
                                                  vp, vp]),
        "epa_guided_begin_prove": (i32, [vp, vp, i32, i32, i32, i32, ctypes.c_float, i32, ctypes.c_int64, i32, vp, vp,
                                         vp]),
        "epa_guided_begin_prove_device": (i32, [vp, vp, i32, i32, i32, i32, ctypes.c_float, i32, ctypes.c_int64, i32,
                                                vp, vp, vp]),
        "epa_guided_proof": (i32, [vp, vp, vp]),
        "epa_guided_proof_device": (i32, [vp, vp, vp]),
        "epa_guided_decided": (i32, [vp, vp, vp]),
        "epa_guided_decided_device": (i32, [vp, vp, vp]),
        "epa_gumbel_begin": (i32, [vp, vp, i32, i32, i32, ctypes.c_float, ctypes.c_float, vp, vp, vp, vp]),
        "epa_gumbel_begin_device": (i32, [vp, vp, i32, i32, i32, ctypes.c_float, ctypes.c_float, vp, vp, vp, vp]),
        "epa_gumbel_begin_batch": (i32, [vp, vp, i32, i32, i32, i32, ctypes.c_float, ctypes.c_float, vp, vp, vp, vp]),
        "epa_gumbel_begin_batch_device": (i32, [vp, vp, i32, i32, i32, i32, ctypes.c_float, ctypes.c_float, vp, vp, vp,
                                                vp]),
        "epa_gumbel_advance": (i32, [vp, vp, vp, i32, vp, vp, vp]),
        "epa_gumbel_advance_device": (i32, [vp, vp, vp, i32, vp, vp, vp]),
        "epa_gumbel_result": (i32, [vp, vp, vp, vp, vp]),
        "epa_gumbel_result_device": (i32, [vp, vp, vp, vp, vp]),
        "epa_net_create": (i32, [i32, vp, ctypes.c_size_t, P(vp)]),
        "epa_net_destroy": (i32, [vp]),
        "epa_net_eval": (i32, [vp, vp, i32, i32, vp, vp, vp, vp, vp]),
        "epa_net_eval_device": (i32, [vp, vp, i32, i32, vp, vp, vp, vp, vp]),
        "epa_net_run": (i32, [vp, vp, i32, vp, vp, vp, P(i32)]),
        "epa_net_run_device": (i32, [vp, vp, i32, vp, vp, vp, P(i32)]),
        "epa_selfplay_begin": (i32, [vp, vp, P(SelfplayOptions)]),
        "epa_selfplay_run": (i32, [vp, i32]),
        "epa_selfplay_run_device": (i32, [vp, i32]),
        "epa_selfplay_stats": (i32, [vp, P(ctypes.c_int64)]),
        "epa_selfplay_end": (i32, [vp]),
        "epa_selfplay_begin_ex": (i32, [vp, vp, vp, P(SelfplayOptions), P(SelfplayExtra)]),
        "epa_selfplay_noise": (i32, [vp, vp]),
        "epa_net_eval_pair": (i32, [vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp]),
        "epa_net_eval_pair_device": (i32, [vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp]),
        "epa_arena_begin": (i32, [vp, vp, vp, P(SelfplayOptions)]),
        "epa_arena_stats": (i32, [vp, P(ctypes.c_int64)]),
        "epa_record_begin": (i32, [vp, i32, i32, ctypes.c_uint32]),
        "epa_record_shape": (i32, [vp, P(i32)]),
        "epa_record_add": (i32, [vp, vp, i32, vp]),
        "epa_record_add_device": (i32, [vp, vp, i32, vp]),
        "epa_record_finish": (i32, [vp, vp, i32, vp, vp]),
        "epa_record_finish_device": (i32, [vp, vp, i32, vp, vp]),
        "epa_record_drain": (i32, [vp, i32, vp, vp, vp, vp, vp, vp, vp, P(i32)]),
        "epa_record_view_device": (i32, [vp, P(vp), P(vp)]),
        "epa_record_clear": (i32, [vp]),
        "epa_record_discard": (i32, [vp, vp, i32]),
        "epa_record_counters": (i32, [vp, P(ctypes.c_int64)]),
        "epa_record_end": (i32, [vp]),
        "epa_rollout_begin": (i32, [vp, i32, i32, ctypes.c_uint32]),
        "epa_rollout_shape": (i32, [vp, P(ctypes.c_int64)]),
        "epa_rollout_reset": (i32, [vp, i32, P(vp), i32, i32, P(i32)]),
        "epa_rollout_step": (i32, [vp, vp, P(vp), i32, i32, P(i32)]),
        "epa_rollout_step_device": (i32, [vp, vp, vp, P(vp), i32, P(i32)]),
        "epa_rollout_view_device": (i32, [vp, P(vp), i32]),
        "epa_rollout_batch": (i32, [vp, P(vp), i32]),
        "epa_rollout_gae": (i32, [vp, vp, ctypes.c_float, ctypes.c_float, vp, vp]),
        "epa_rollout_gae_device": (i32, [vp, vp, ctypes.c_float, ctypes.c_float, vp, vp]),
        "epa_rollout_episodes": (i32, [vp, i32, vp, vp, vp, vp, P(i32)]),
        "epa_rollout_episodes_view_device": (i32, [vp, P(vp), P(vp)]),
        "epa_rollout_moments": (i32, [vp, vp, P(vp)]),
        "epa_rollout_next": (i32, [vp]),
        "epa_rollout_counters": (i32, [vp, P(ctypes.c_int64)]),
        "epa_rollout_end": (i32, [vp]),
        "epa_actor_begin": (i32, [vp, vp, ctypes.c_size_t, ctypes.c_uint64, ctypes.c_uint32, i32, vp, vp]),
        "epa_actor_shape": (i32, [vp, P(ctypes.c_int64)]),
        "epa_actor_end": (i32, [vp]),
        "epa_actor_eval": (i32, [vp, vp, i32, ctypes.c_int64, P(vp), i32, vp, vp, vp]),
        "epa_actor_eval_device": (i32, [vp, vp, i32, ctypes.c_int64, P(vp), i32, vp, vp, vp]),
        "epa_actor_view_device": (i32, [vp, P(vp), P(vp)]),
        "epa_actor_batch": (i32, [vp, vp, vp]),
        "epa_rollout_collect": (i32, [vp, i32]),
        "epa_rollout_collect_device": (i32, [vp, i32]),
        "epa_atari_post_create": (i32, [i32] * 8 + [P(vp)]),
        "epa_atari_post_create_ex": (i32, [i32] * 8 + [vp, i32, P(vp)]),
        "epa_atari_create": (i32, [P(EpaAtariConfig), P(vp)]),
        "epa_atari_num_actions": (i32, [P(EpaAtariConfig), P(i32)]),
        "epa_pool_state_keys": (i32, [vp, P(EpaKeyInfo), i32, P(i32)]),
        "epa_pool_action_keys": (i32, [vp, P(EpaKeyInfo), i32, P(i32)]),
        "epa_atari_post_destroy": (i32, [vp]),
        "epa_atari_post_push": (i32, [vp, vp, i32, vp, vp, vp]),
        "epa_atari_post_push_device": (i32, [vp, vp, i32, vp, vp, vp]),
        "epa_atari_post_stream": (vp, [vp]),
        "epa_last_error": (cp, []),
        "epa_version": (cp, []),
        "epa_device_count": (i32, [P(i32)]),
        "epa_host_alloc": (vp, [ctypes.c_size_t]),
        "epa_host_free": (None, [vp]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


EXPORTED_SYMBOLS = [
    "epa_num_families", "epa_family_name", "epa_describe_state",
    "epa_describe_action", "epa_family_players", "epa_describe_state_players",
    "epa_create", "epa_destroy", "epa_send", "epa_reset",
    "epa_recv", "epa_recv_layout", "epa_recv_block", "epa_send_into", "epa_recv_into", "epa_pending_rows",
    "epa_send_device", "epa_recv_device", "epa_step_device", "epa_wait_stream", "epa_consumer_wait",
    "epa_stream", "epa_synchronize", "epa_set_timing", "epa_kernel_time_ms",
    "epa_state_dim", "epa_get_state", "epa_set_state", "epa_render_size", "epa_render", "epa_render_device",
    "epa_snapshot_bytes", "epa_snapshot", "epa_restore", "epa_snapshot_device", "epa_restore_device", "epa_fork",
    "epa_playout", "epa_playout_device", "epa_search_actions", "epa_search", "epa_search_device",
    "epa_solve", "epa_solve_device", "epa_solve_table", "epa_solve_table_device",
    "epa_guided_shape", "epa_guided_begin", "epa_guided_begin_device", "epa_guided_advance",
    "epa_guided_advance_device", "epa_guided_result", "epa_guided_result_device", "epa_guided_end",
    "epa_guided_begin_nodes", "epa_guided_begin_nodes_device", "epa_guided_reroot", "epa_guided_reroot_device",
    "epa_guided_begin_wide", "epa_guided_begin_wide_device",
    "epa_guided_begin_tactics", "epa_guided_begin_tactics_device", "epa_guided_decided", "epa_guided_decided_device",
    "epa_guided_begin_prove", "epa_guided_begin_prove_device", "epa_guided_proof", "epa_guided_proof_device",
    "epa_gumbel_begin", "epa_gumbel_begin_device", "epa_gumbel_advance", "epa_gumbel_advance_device",
    "epa_gumbel_result", "epa_gumbel_result_device", "epa_gumbel_begin_batch", "epa_gumbel_begin_batch_device",
    "epa_net_create", "epa_net_destroy", "epa_net_eval", "epa_net_eval_device", "epa_net_run", "epa_net_run_device",
    "epa_record_begin", "epa_record_shape", "epa_record_add", "epa_record_add_device", "epa_record_finish",
    "epa_record_finish_device", "epa_record_drain", "epa_record_view_device", "epa_record_clear",
    "epa_record_discard", "epa_record_counters", "epa_record_end",
    "epa_rollout_begin", "epa_rollout_shape", "epa_rollout_reset", "epa_rollout_step", "epa_rollout_step_device",
    "epa_rollout_view_device", "epa_rollout_batch", "epa_rollout_gae", "epa_rollout_gae_device",
    "epa_rollout_episodes", "epa_rollout_episodes_view_device", "epa_rollout_moments", "epa_rollout_next",
    "epa_rollout_counters", "epa_rollout_end",
    "epa_actor_begin", "epa_actor_shape", "epa_actor_end", "epa_actor_eval", "epa_actor_eval_device",
    "epa_actor_view_device", "epa_actor_batch", "epa_rollout_collect", "epa_rollout_collect_device",
    "epa_selfplay_begin", "epa_selfplay_run", "epa_selfplay_run_device", "epa_selfplay_stats", "epa_selfplay_end",
    "epa_net_eval_pair", "epa_net_eval_pair_device", "epa_arena_begin", "epa_arena_stats",
    "epa_selfplay_begin_ex", "epa_selfplay_noise",
    "epa_atari_post_create",
    "epa_atari_post_create_ex", "epa_atari_create", "epa_atari_num_actions",
    "epa_pool_state_keys", "epa_pool_action_keys",
    "epa_atari_post_destroy", "epa_atari_post_push",
    "epa_atari_post_push_device", "epa_atari_post_stream", "epa_last_error",
    "epa_version", "epa_device_count", "epa_host_alloc", "epa_host_free",
]


def check(code: int) -> None:
    """Map C-ABI error classes onto the exceptions the reference raises
    (std::invalid_argument -> ValueError, std::runtime_error -> RuntimeError)."""
    if code == EPA_OK:
        return
    msg = lib().epa_last_error().decode()
    if code == EPA_ERR_INVALID:
        raise ValueError(msg)
    raise RuntimeError(msg)


def snapshot_header(blob: np.ndarray) -> tuple[int, int]:
    """(env count, byte count) a snapshot blob's header states.  ValueError for a blob shorter than a header, or
    shorter than its header says: checked here, before any native call sees the blob."""
    blob = np.asarray(blob)
    if blob.dtype != np.uint8 or blob.ndim != 1:
        raise ValueError("snapshot blob must be a one-dimensional uint8 array")
    if blob.nbytes < SNAP_HEADER_BYTES:
        raise ValueError(f"snapshot blob of {blob.nbytes} bytes is shorter than a header")
    k = int(blob[20:24].view("<i4")[0])
    total = int(blob[48:56].view("<u8")[0])
    if blob.nbytes < total:
        raise ValueError(f"snapshot blob of {blob.nbytes} bytes is shorter than its header says ({total})")
    return k, total


def check_playout(env_ids: Any, repeats: int, max_plies: int, commit: bool) -> np.ndarray:
    """The ids of a playout call as a flat int32 array, after the argument checks every layer makes before the native
    call: ValueError for repeats outside 1 .. 4096, max_plies outside 0 .. 256, no ids, and a commit with
    repeats != 1 or with an id that repeats.  (Ids outside the pool are the engine's to refuse.)"""
    ids = np.ascontiguousarray(env_ids, dtype=np.int32).reshape(-1)
    if not 1 <= int(repeats) <= PLAYOUT_MAX_REPEATS:
        raise ValueError(f"playout: repeats = {repeats} must be 1 .. {PLAYOUT_MAX_REPEATS}")
    if not 0 <= int(max_plies) <= PLAYOUT_MAX_PLIES:
        raise ValueError(f"playout: max_plies = {max_plies} must be 0 .. {PLAYOUT_MAX_PLIES}")
    if len(ids) == 0:
        raise ValueError("playout env_ids must not be empty")
    if commit:
        if int(repeats) != 1:
            raise ValueError("playout: commit takes repeats = 1")
        if len(np.unique(ids)) != len(ids):
            raise ValueError("playout: commit takes env_ids that do not repeat")
    return ids


def check_record(capacity: int, max_plies: int, symmetries: Any) -> tuple[int, int, bool]:
    """A recorder's (capacity, max_plies, symmetries) after the argument checks every layer makes before the native
    call: ValueError for a capacity that is no integer of at least 1 (or past int32), max_plies outside 0 .. 256 and a
    `symmetries` that is no bool.  (The 2 GiB limit of the staging and the samples is the engine's to refuse.)"""
    if isinstance(capacity, bool) or int(capacity) != capacity or not 1 <= int(capacity) < 2**31:
        raise ValueError(f"recorder: capacity = {capacity} must be at least 1")
    if isinstance(max_plies, bool) or int(max_plies) != max_plies or not 0 <= int(max_plies) <= RECORD_MAX_PLIES:
        raise ValueError(f"recorder: max_plies = {max_plies} must be 0 .. {RECORD_MAX_PLIES}")
    if not isinstance(symmetries, (bool, np.bool_)):
        raise ValueError(f"recorder: symmetries = {symmetries!r} must be a bool")
    return int(capacity), int(max_plies), bool(symmetries)


def check_record_ids(what: str, env_ids: Any) -> np.ndarray:
    """The ids of a recorder call as a flat int32 array: ValueError for no ids and for an id listed twice.  (Ids
    outside the pool are the engine's to refuse.)"""
    ids = np.ascontiguousarray(env_ids, dtype=np.int32).reshape(-1)
    if len(ids) == 0:
        raise ValueError(f"{what} env_ids must not be empty")
    if len(np.unique(ids)) != len(ids):
        raise ValueError(f"{what}: env_ids must not repeat")
    return ids


def check_record_add(policy: Any, k: int, actions: int) -> np.ndarray:
    """add's policy rows as a contiguous float32 [k, A] array (any values: the recorder cleans them)."""
    policy = np.ascontiguousarray(policy, dtype=np.float32)
    if policy.shape != (k, actions):
        raise ValueError(f"recorder add: policy of shape {policy.shape} for {k} envs of {actions} actions")
    return policy


def check_record_finish(reward: Any, done: Any, k: int) -> tuple[np.ndarray, np.ndarray]:
    """finish's rows as the step returned them: reward float32 [k, 2] (or [2 k], the per-player rows) and done [k]."""
    reward = np.ascontiguousarray(reward, dtype=np.float32)
    done = np.ascontiguousarray(done)
    if reward.size != 2 * k or reward.ndim > 2 or (reward.ndim == 2 and reward.shape != (k, 2)):
        raise ValueError(f"recorder finish: reward of shape {reward.shape} for {k} envs of 2 players")
    if done.shape != (k,):
        raise ValueError(f"recorder finish: done of shape {done.shape} for {k} envs")
    return reward.reshape(k, 2), np.ascontiguousarray(done != 0, dtype=np.uint8)


def rollout_bytes(num_envs: int, horizon: int, episodes: int, obs_bytes: int, action_bytes: int) -> int:
    """Bytes of a rollout collector's buffers (csrc/rollout.hip.h: RolloutBytes): obs [T+1, N], action, reward and the
    three flag arrays [T, N], and 24 bytes per episode row."""
    return (horizon + 1) * num_envs * obs_bytes + horizon * num_envs * (action_bytes + 4 + 3) + episodes * 24


def check_rollout(horizon: Any, episodes: Any = 0, moments: Any = False, num_envs: int = 1, obs_bytes: int = 0,
                  action_bytes: int = 0, values: Any = None, gamma: Any = None, lam: Any = None,
                  actor: bool = False) -> tuple:
    """A rollout collector's arguments after the checks every layer makes before the native call, with no device:
    ValueError for a horizon that is no integer of at least 1, episodes that is no integer of at least 0, a `moments`
    that is no bool, and buffers above the 2 GiB limit (`num_envs` envs of `obs_bytes` observation and `action_bytes`
    action bytes each).  With `values` (and `gamma`, `lam`) also gae's arguments: values must be a float32 array of
    shape [horizon + 1, num_envs], gamma and lam numbers in [0, 1].  Returns (horizon, episodes, moments), with values
    (horizon, episodes, moments, values, gamma, lam) -- gamma and lam rounded to float32.  `actor`: the limit also
    counts the logp [T, N] and value [T + 1, N] float32 buffers an attached actor adds (csrc/actor.hip.h)."""
    if isinstance(horizon, (bool, np.bool_)) or not isinstance(horizon, (int, np.integer)) or not 1 <= int(horizon) < 2**31:
        raise ValueError(f"rollout: horizon = {horizon!r} must be an integer of at least 1")
    if isinstance(episodes, (bool, np.bool_)) or not isinstance(episodes, (int, np.integer)) \
            or not 0 <= int(episodes) < 2**31:
        raise ValueError(f"rollout: episodes = {episodes!r} must be an integer of at least 0")
    if not isinstance(moments, (bool, np.bool_)):
        raise ValueError(f"rollout: moments = {moments!r} must be a bool")
    horizon, episodes, moments = int(horizon), int(episodes), bool(moments)
    total = rollout_bytes(int(num_envs), horizon, episodes, int(obs_bytes), int(action_bytes))
    if actor:
        total += 4 * horizon * int(num_envs) + 4 * (horizon + 1) * int(num_envs)
    if total > ROLLOUT_MAX_BYTES:
        raise ValueError(f"rollout: {num_envs} envs over a horizon of {horizon} with {episodes} episode rows need "
                         f"{total} bytes, above the limit of 2 GiB")
    if values is None:
        return horizon, episodes, moments
    if not isinstance(values, np.ndarray) or values.dtype != np.float32:
        raise ValueError(f"rollout gae: values must be a float32 array, got {getattr(values, 'dtype', type(values))}")
    if values.shape != (horizon + 1, int(num_envs)):
        raise ValueError(f"rollout gae: values of shape {values.shape} for [{horizon + 1}, {int(num_envs)}]")
    out = []
    for name, x in (("gamma", gamma), ("lam", lam)):
        if isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, float, np.integer, np.floating)) \
                or not 0.0 <= float(x) <= 1.0:
            raise ValueError(f"rollout gae: {name} = {x!r} must be a number in [0, 1]")
        out.append(float(np.float32(x)))
    return horizon, episodes, moments, np.ascontiguousarray(values), out[0], out[1]


def check_search(env_ids: Any, simulations: int, leaf_playouts: int, c_puct: float, max_plies: int) -> np.ndarray:
    """The ids of a search call as a flat int32 array, after the argument checks every layer makes before the native
    call: ValueError for simulations outside 1 .. 4096, leaf_playouts outside 1 .. 64, simulations * leaf_playouts
    above 4096 (the leaf playouts are repeats of `playout`), max_plies outside 0 .. 256, a c_puct that is not finite
    or negative, and no ids.  (Ids outside the pool and the size of the tree scratch are the engine's to refuse.)"""
    ids = np.ascontiguousarray(env_ids, dtype=np.int32).reshape(-1)
    if not 1 <= int(simulations) <= SEARCH_MAX_SIMULATIONS:
        raise ValueError(f"search: simulations = {simulations} must be 1 .. {SEARCH_MAX_SIMULATIONS}")
    if not 1 <= int(leaf_playouts) <= SEARCH_MAX_LEAF_PLAYOUTS:
        raise ValueError(f"search: leaf_playouts = {leaf_playouts} must be 1 .. {SEARCH_MAX_LEAF_PLAYOUTS}")
    if int(simulations) * int(leaf_playouts) > PLAYOUT_MAX_REPEATS:
        raise ValueError(f"search: simulations * leaf_playouts = {int(simulations) * int(leaf_playouts)} must be at "
                         f"most {PLAYOUT_MAX_REPEATS}")
    if not 0 <= int(max_plies) <= PLAYOUT_MAX_PLIES:
        raise ValueError(f"search: max_plies = {max_plies} must be 0 .. {PLAYOUT_MAX_PLIES}")
    with np.errstate(over="ignore"):
        c = np.float32(c_puct)
    if not np.isfinite(c) or c < 0:
        raise ValueError(f"search: c_puct = {c_puct} must be finite and >= 0")
    if len(ids) == 0:
        raise ValueError("search env_ids must not be empty")
    return ids


def check_solve(env_ids: Any, depth: int, max_nodes: int, table_bits: int = 0) -> np.ndarray:
    """The ids of a solve call as a flat int32 array, after the argument checks every layer makes before the native
    call: ValueError for a depth outside 0 .. 128, max_nodes below 1 (or past int64), table_bits outside 0 .. 16 and
    no ids.  (Ids outside the pool and the size of the stacks and tables are the engine's to refuse.)"""
    ids = np.ascontiguousarray(env_ids, dtype=np.int32).reshape(-1)
    if isinstance(depth, bool) or int(depth) != depth or not 0 <= int(depth) <= SOLVE_MAX_DEPTH:
        raise ValueError(f"solve: depth = {depth} must be 0 .. {SOLVE_MAX_DEPTH}")
    if isinstance(max_nodes, bool) or int(max_nodes) != max_nodes or not 1 <= int(max_nodes) < 2**63:
        raise ValueError(f"solve: max_nodes = {max_nodes} must be at least 1")
    if (isinstance(table_bits, bool) or int(table_bits) != table_bits
            or not 0 <= int(table_bits) <= SOLVE_MAX_TABLE_BITS):
        raise ValueError(f"solve: table_bits = {table_bits} must be in 0 .. {SOLVE_MAX_TABLE_BITS}")
    if len(ids) == 0:
        raise ValueError("solve env_ids must not be empty")
    return ids


def check_guided(env_ids: Any, simulations: int, c_puct: float) -> np.ndarray:
    """The ids of a guided_begin call as a flat int32 array, after the argument checks every layer makes before the
    native call: ValueError for simulations outside 1 .. 4096, a c_puct that is not finite or negative, and no ids.
    (Ids outside the pool and the size of the trees are the engine's to refuse.)"""
    ids = np.ascontiguousarray(env_ids, dtype=np.int32).reshape(-1)
    if not 1 <= int(simulations) <= SEARCH_MAX_SIMULATIONS:
        raise ValueError(f"guided_begin: simulations = {simulations} must be 1 .. {SEARCH_MAX_SIMULATIONS}")
    with np.errstate(over="ignore"):
        c = np.float32(c_puct)
    if not np.isfinite(c) or c < 0:
        raise ValueError(f"guided_begin: c_puct = {c_puct} must be finite and >= 0")
    if len(ids) == 0:
        raise ValueError("guided_begin env_ids must not be empty")
    return ids


def check_guided_nodes(simulations: int, nodes: Any) -> int:
    """The node capacity per root of a guided_begin call: `nodes` (None or 0: simulations + 1) after its check:
    ValueError outside simulations + 1 .. 8192."""
    if nodes is None or int(nodes) == 0:
        return int(simulations) + 1
    if not int(simulations) + 1 <= int(nodes) <= GUIDED_MAX_NODES:
        raise ValueError(f"guided_begin: nodes = {nodes} must be simulations + 1 = {int(simulations) + 1} .. "
                         f"{GUIDED_MAX_NODES}")
    return int(nodes)


def check_guided_width(width: Any) -> int:
    """The width (slots per root) of a guided_begin call after its check: ValueError outside 1 .. 32.  None: 0, a plain
    session."""
    if width is None:
        return 0
    if isinstance(width, bool) or int(width) != width or not 1 <= int(width) <= GUIDED_MAX_WIDTH:
        raise ValueError(f"guided_begin: width = {width} must be 1 .. {GUIDED_MAX_WIDTH}")
    return int(width)


def check_guided_tactics(tactics: Any, tactics_nodes: Any) -> tuple[int, int]:
    """(D, M) of a guided_begin call's exact leaf status after their checks: ValueError for a `tactics` outside 0 .. 16
    (None or 0: off) or a `tactics_nodes` outside 1 .. 2^20."""
    if tactics is None:
        tactics = 0
    if isinstance(tactics, bool) or int(tactics) != tactics or not 0 <= int(tactics) <= GUIDED_MAX_TACTICS:
        raise ValueError(f"guided_begin: tactics = {tactics} must be 0 .. {GUIDED_MAX_TACTICS}")
    if (isinstance(tactics_nodes, bool) or int(tactics_nodes) != tactics_nodes
            or not 1 <= int(tactics_nodes) <= GUIDED_MAX_TACTICS_NODES):
        raise ValueError(f"guided_begin: tactics_nodes = {tactics_nodes} must be 1 .. {GUIDED_MAX_TACTICS_NODES}")
    return int(tactics), int(tactics_nodes)


def check_guided_prove(prove: Any) -> bool:
    """`prove` of a guided_begin call after its check: ValueError unless it is a bool (None: False)."""
    if prove is None:
        return False
    if not isinstance(prove, (bool, np.bool_)):
        raise ValueError(f"guided_begin: prove = {prove!r} must be True or False")
    return bool(prove)


def check_guided_wide_rows(priors: Any, values: Any, k: int, width: int, actions: int) -> tuple[np.ndarray, np.ndarray]:
    """The rows of a host-form guided_advance of a wide session, given with the slot axis ([k, W, A] and [k, W]) or
    flattened ([k W, A] and [k W]), as contiguous float32 arrays [k W, A] and [k W] after the checks of
    `check_guided_rows`."""
    priors = np.ascontiguousarray(priors, dtype=np.float32)
    if priors.shape not in ((k, width, actions), (k * width, actions)):
        raise ValueError(f"guided_advance: priors of shape {priors.shape} for a session of [{k}, {width}, {actions}]")
    values = np.ascontiguousarray(values, dtype=np.float32)
    if values.shape not in ((k, width), (k * width,)):
        raise ValueError(f"guided_advance: values of shape {values.shape} for a session of [{k}, {width}]")
    return check_guided_rows(priors.reshape(k * width, actions), values.reshape(-1), k * width, actions)


def check_guided_reroot(actions: Any, k: int, n_actions: int, simulations: int, nodes: int,
                        device: bool = False) -> np.ndarray:
    """The checks of a guided_reroot call that every layer makes before the native call: ValueError for simulations
    outside 1 .. 4096 or above nodes - 1, and, in the host form, for another number of rows than the session's and an
    action outside 0 .. A-1; returns the actions as a contiguous int32 array [k].  (The device form cannot look at its
    rows -- `actions` is returned as it is; there the kernel ends such a root.)"""
    if not 1 <= int(simulations) <= SEARCH_MAX_SIMULATIONS:
        raise ValueError(f"guided_reroot: simulations = {simulations} must be 1 .. {SEARCH_MAX_SIMULATIONS}")
    if int(simulations) + 1 > int(nodes):
        raise ValueError(f"guided_reroot: simulations = {simulations} need {int(simulations) + 1} nodes, the session "
                         f"has {nodes} per root")
    if device:
        return actions
    actions = np.ascontiguousarray(actions, dtype=np.int32).reshape(-1)
    if actions.shape != (k,):
        raise ValueError(f"guided_reroot: {len(actions)} actions for a session of {k} roots")
    if not ((actions >= 0) & (actions < n_actions)).all():
        raise ValueError(f"guided_reroot: actions must be 0 .. {n_actions - 1}")
    return actions


def check_guided_rows(priors: Any, values: Any, k: int, actions: int) -> tuple[np.ndarray, np.ndarray]:
    """The rows of a host-form guided_advance as contiguous float32 arrays [k, A] and [k]: ValueError for another
    number of rows, a prior that is negative or not finite, a value outside -1 .. 1 or not a number.  (The device form
    cannot look at its rows; there the kernel replaces such entries by 0.)"""
    priors = np.ascontiguousarray(priors, dtype=np.float32)
    values = np.ascontiguousarray(values, dtype=np.float32).reshape(-1)
    if priors.shape != (k, actions):
        raise ValueError(f"guided_advance: priors of shape {priors.shape} for a session of [{k}, {actions}]")
    if values.shape != (k,):
        raise ValueError(f"guided_advance: {len(values)} values for a session of {k} roots")
    if not (np.isfinite(priors) & (priors >= 0)).all():
        raise ValueError("guided_advance: priors must be finite and >= 0")
    if not ((values >= -1) & (values <= 1)).all():
        raise ValueError("guided_advance: values must be in -1 .. 1")
    return priors, values


def check_gumbel(env_ids: Any, simulations: int, max_considered: int, c_visit: float, c_scale: float) -> np.ndarray:
    """The ids of a gumbel_begin call as a flat int32 array, after the argument checks every layer makes before the
    native call: ValueError for simulations outside 1 .. 4096, max_considered below 1 (one above the game's actions
    counts as all of them), a c_visit or c_scale that is not finite or negative, and no ids."""
    ids = np.ascontiguousarray(env_ids, dtype=np.int32).reshape(-1)
    if not 1 <= int(simulations) <= SEARCH_MAX_SIMULATIONS:
        raise ValueError(f"gumbel_begin: simulations = {simulations} must be 1 .. {SEARCH_MAX_SIMULATIONS}")
    if not 1 <= int(max_considered) < 2**31:
        raise ValueError(f"gumbel_begin: max_considered = {max_considered} must be at least 1")
    for name, c in (("c_visit", c_visit), ("c_scale", c_scale)):
        with np.errstate(over="ignore"):
            c32 = np.float32(c)
        if not np.isfinite(c32) or c32 < 0:
            raise ValueError(f"gumbel_begin: {name} = {c} must be finite and >= 0")
    if len(ids) == 0:
        raise ValueError("gumbel_begin env_ids must not be empty")
    return ids


def check_gumbel_noise(gumbel: Any, k: int, actions: int) -> np.ndarray:
    """The Gumbel noise of a host-form gumbel_begin as a contiguous float32 array [k, A]: ValueError for another
    shape or an entry that is not finite."""
    gumbel = np.ascontiguousarray(gumbel, dtype=np.float32)
    if gumbel.shape != (k, actions):
        raise ValueError(f"gumbel_begin: gumbel of shape {gumbel.shape} for a session of [{k}, {actions}]")
    if not np.isfinite(gumbel).all():
        raise ValueError("gumbel_begin: gumbel must be finite")
    return gumbel


def check_gumbel_rows(logits: Any, values: Any, k: int, actions: int) -> tuple[np.ndarray, np.ndarray]:
    """The rows of a host-form gumbel_advance as contiguous float32 arrays [k, A] and [k]: ValueError for another
    number of rows, a logit that is not finite or above 1e30 in magnitude (negative logits are fine), a value outside
    -1 .. 1 or not a number.  (The device form cannot look at its rows; there the kernel replaces such entries by 0.)"""
    with np.errstate(over="ignore"):
        logits = np.ascontiguousarray(logits, dtype=np.float32)
    values = np.ascontiguousarray(values, dtype=np.float32).reshape(-1)
    if logits.shape != (k, actions):
        raise ValueError(f"gumbel_advance: logits of shape {logits.shape} for a session of [{k}, {actions}]")
    if values.shape != (k,):
        raise ValueError(f"gumbel_advance: {len(values)} values for a session of {k} roots")
    if not (np.abs(logits) <= np.float32(1e30)).all():
        raise ValueError("gumbel_advance: logits must be finite and at most 1e30 in magnitude")
    if not ((values >= -1) & (values <= 1)).all():
        raise ValueError("gumbel_advance: values must be in -1 .. 1")
    return logits, values


def check_gumbel_batch(batch: Any) -> int:
    """The batch (slots per root) of a gumbel_begin call after its check: ValueError outside 1 .. 32.  None: 0, a plain
    session."""
    if batch is None:
        return 0
    if isinstance(batch, bool) or int(batch) != batch or not 1 <= int(batch) <= GUMBEL_MAX_BATCH:
        raise ValueError(f"gumbel_begin: batch = {batch} must be 1 .. {GUMBEL_MAX_BATCH}")
    return int(batch)


def check_net_advances(advances: Any) -> int:
    """The `advances` of a net_run call after its check: None is 0 (until the round is complete); ValueError for
    anything but an integer >= 1 (the engine checks it against the session's simulations)."""
    if advances is None:
        return 0
    if isinstance(advances, bool) or int(advances) != advances or int(advances) < 1:
        raise ValueError(f"net_run: advances = {advances} must be at least 1, or None")
    return int(advances)


class SelfplayOptions(ctypes.Structure):
    """epa_selfplay_options (include/envpool_amd.h)."""

    _fields_ = [("policy", ctypes.c_int32), ("simulations", ctypes.c_int32), ("max_considered", ctypes.c_int32),
                ("batch", ctypes.c_int32), ("c_visit", ctypes.c_float), ("c_scale", ctypes.c_float),
                ("c_puct", ctypes.c_float), ("width", ctypes.c_int32), ("tactics", ctypes.c_int32),
                ("prove", ctypes.c_int32), ("tactics_nodes", ctypes.c_int64), ("seed", ctypes.c_uint64),
                ("noise", ctypes.c_int32), ("sample_plies", ctypes.c_int32), ("record", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


class SelfplayExtra(ctypes.Structure):
    """epa_selfplay_extra (include/envpool_amd.h): the PUCT exploration of a driver or an arena."""

    _fields_ = [("dirichlet_alpha", ctypes.c_float), ("dirichlet_eps", ctypes.c_float),
                ("temperature", ctypes.c_float), ("reserved", ctypes.c_int32)]


SELFPLAY_GUMBEL = 0  # EPA_SELFPLAY_GUMBEL / EPA_SELFPLAY_PUCT: the policies of a self-play driver
SELFPLAY_PUCT = 1
# the options of `selfplay` that belong to one policy, with the value that means "not given"
_SELFPLAY_GUMBEL_ONLY = {"max_considered": None, "c_visit": None, "c_scale": None, "batch": 1, "noise": None}
_SELFPLAY_PUCT_ONLY = {"c_puct": None, "width": 1, "tactics": 0, "tactics_nodes": None, "prove": False,
                       "sample_plies": 0, "dirichlet_alpha": 0.0, "dirichlet_eps": 0.25, "temperature": 1.0}
DIRICHLET_MAX_ALPHA = 100.0  # csrc/pgx_dirichlet.hip.h: kDirichletMaxAlpha, kTemperatureMin, kTemperatureMax
TEMPERATURE_RANGE = (0.05, 20.0)


def check_selfplay_extra(policy: Any = "puct", dirichlet_alpha: Any = 0.0, dirichlet_eps: Any = 0.25,
                         temperature: Any = 1.0) -> SelfplayExtra:
    """The PUCT exploration of a selfplay_begin or arena_begin call as the C struct (epa_selfplay_extra), after the
    checks every layer makes before the native call.  ValueError for a `dirichlet_alpha` that is not finite or outside
    0 .. 100, a `dirichlet_eps` outside 0 .. 1, a `temperature` outside 0.05 .. 20 -- as float32, the values the
    engine sees -- and for any of them other than its default with policy='gumbel'.  Without noise
    (`dirichlet_alpha == 0`) the struct's eps is 0: {0, 0, 1, 0} is the plain driver."""
    if policy not in ("gumbel", "puct"):
        raise ValueError(f"selfplay: policy = {policy!r} must be 'puct' or 'gumbel'")
    given = dict(dirichlet_alpha=dirichlet_alpha, dirichlet_eps=dirichlet_eps, temperature=temperature)
    vals = {}
    for name, value in given.items():
        if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, float, np.integer, np.floating)):
            raise ValueError(f"selfplay: {name} = {value!r} must be a number")
        with np.errstate(over="ignore"):
            vals[name] = float(np.float32(value))
    if policy == "gumbel":
        stray = sorted(n for n in given if not vals[n] == float(np.float32(_SELFPLAY_PUCT_ONLY[n])))
        if stray:
            raise ValueError(f"selfplay: {stray} are arguments of policy='puct'")
        return SelfplayExtra(0.0, 0.0, 1.0, 0)
    a, e, t = vals["dirichlet_alpha"], vals["dirichlet_eps"], vals["temperature"]
    if not 0.0 <= a <= DIRICHLET_MAX_ALPHA:
        raise ValueError(f"selfplay: dirichlet_alpha = {dirichlet_alpha} must be finite and in 0 .. 100")
    if not 0.0 <= e <= 1.0:
        raise ValueError(f"selfplay: dirichlet_eps = {dirichlet_eps} must be in 0 .. 1")
    if not float(np.float32(TEMPERATURE_RANGE[0])) <= t <= TEMPERATURE_RANGE[1]:
        raise ValueError(f"selfplay: temperature = {temperature} must be in 0.05 .. 20")
    return SelfplayExtra(a, e if a > 0.0 else 0.0, t, 0)


def check_selfplay(policy: Any = "gumbel", simulations: Any = 32, max_considered: Any = None, c_visit: Any = None,
                   c_scale: Any = None, batch: Any = 1, c_puct: Any = None, width: Any = 1, tactics: Any = 0,
                   tactics_nodes: Any = None, prove: Any = False, seed: Any = 0, noise: Any = None,
                   sample_plies: Any = 0, record: Any = True, dirichlet_alpha: Any = 0.0, dirichlet_eps: Any = 0.25,
                   temperature: Any = 1.0) -> SelfplayOptions:
    """The options of a selfplay_begin call as the C struct, after the checks every layer makes before the native call.
    ValueError for an unknown policy; for an option of the other policy, worded as `guided_search` words it; for a seed
    outside 0 .. 2^64 - 1, a `noise` or `record` that is no bool, a `sample_plies` that is no integer >= 0; and for the
    option values the policy's own begin refuses (`check_gumbel`, `check_gumbel_batch`, `check_guided`,
    `check_guided_width`, `check_guided_tactics`, `check_guided_prove`).  Defaults are the searches': max_considered 16,
    c_visit 50, c_scale 0.1, c_puct 1.25, noise on.  `dirichlet_alpha`, `dirichlet_eps` and `temperature` are
    `check_selfplay_extra`'s (policy='puct'), which makes their struct."""
    given = dict(max_considered=max_considered, c_visit=c_visit, c_scale=c_scale, batch=batch, noise=noise,
                 c_puct=c_puct, width=width, tactics=tactics, tactics_nodes=tactics_nodes, prove=prove,
                 sample_plies=sample_plies, dirichlet_alpha=dirichlet_alpha, dirichlet_eps=dirichlet_eps,
                 temperature=temperature)
    if policy not in ("gumbel", "puct"):
        raise ValueError(f"selfplay: policy = {policy!r} must be 'puct' or 'gumbel'")
    check_selfplay_extra(policy, dirichlet_alpha, dirichlet_eps, temperature)
    theirs = _SELFPLAY_PUCT_ONLY if policy == "gumbel" else _SELFPLAY_GUMBEL_ONLY
    stray = sorted(name for name, unset in theirs.items() if given[name] is not None and given[name] != unset)
    if stray:
        other = "puct" if policy == "gumbel" else "gumbel"
        raise ValueError(f"selfplay: {stray} are arguments of policy='{other}'")
    if isinstance(seed, bool) or int(seed) != seed or not 0 <= int(seed) < 2**64:
        raise ValueError(f"selfplay: seed = {seed} must be an integer in 0 .. 2^64 - 1")
    if not isinstance(record, (bool, np.bool_)):
        raise ValueError(f"selfplay: record = {record!r} must be True or False")
    o = SelfplayOptions()
    o.seed, o.record, o.simulations = int(seed), int(bool(record)), int(simulations)
    if policy == "gumbel":
        if noise is None:
            noise = True
        if not isinstance(noise, (bool, np.bool_)):
            raise ValueError(f"selfplay: noise = {noise!r} must be True or False")
        m = 16 if max_considered is None else max_considered
        cv, cs = 50.0 if c_visit is None else c_visit, 0.1 if c_scale is None else c_scale
        check_gumbel(np.zeros(1, dtype=np.int32), simulations, m, cv, cs)
        b = check_gumbel_batch(batch)
        o.policy, o.max_considered, o.c_visit, o.c_scale = SELFPLAY_GUMBEL, int(m), float(cv), float(cs)
        o.batch, o.noise = (b if b > 1 else 0), int(bool(noise))
        return o  # (every PUCT field stays 0: the engine refuses anything else)
    if isinstance(sample_plies, bool) or int(sample_plies) != sample_plies or not 0 <= int(sample_plies) < 2**31:
        raise ValueError(f"selfplay: sample_plies = {sample_plies} must be an integer >= 0")
    c = 1.25 if c_puct is None else c_puct
    check_guided(np.zeros(1, dtype=np.int32), simulations, c)
    w = check_guided_width(width)
    t, tn = check_guided_tactics(tactics, GUIDED_TACTICS_NODES if tactics_nodes is None else tactics_nodes)
    o.policy, o.c_puct, o.width, o.tactics, o.tactics_nodes = SELFPLAY_PUCT, float(c), (w if w > 1 else 0), t, tn
    o.prove, o.sample_plies = int(check_guided_prove(prove)), int(sample_plies)
    return o


ARENA_MAX_ROWS = 1 << 20  # rows of one pair evaluation (csrc/pgx_arena.hip.h: kArenaMaxRows)


def check_arena(net_a: Any, net_b: Any, record: Any = False, **options: Any) -> SelfplayOptions:
    """The options of an arena_begin call as the C struct, after the checks every layer makes before the native call:
    ValueError for a net that is no `envpool_amd.pgx.net.Net`, for two nets that differ in inputs (F) or actions (A) --
    hidden width and blocks may differ --, and for everything `check_selfplay` refuses.  `record` defaults to False."""
    for name, net in (("net_a", net_a), ("net_b", net_b)):
        if not getattr(net, "_is_epa_net", False):
            raise ValueError(f"arena: {name} must be an envpool_amd.pgx.net.Net")
    if int(net_a.inputs) != int(net_b.inputs) or int(net_a.actions) != int(net_b.actions):
        raise ValueError(f"arena: net_a has F = {int(net_a.inputs)}, A = {int(net_a.actions)} and net_b F = "
                         f"{int(net_b.inputs)}, A = {int(net_b.actions)}: the two nets must agree in both")
    return check_selfplay(record=record, **options)


def selfplay_extra_of(options: dict) -> SelfplayExtra:
    """`check_selfplay_extra` of a dict of `check_selfplay`'s options."""
    return check_selfplay_extra(options.get("policy", "gumbel"), options.get("dirichlet_alpha", 0.0),
                                options.get("dirichlet_eps", 0.25), options.get("temperature", 1.0))


def check_arena_side(side: Any, rows: int) -> np.ndarray:
    """The side bytes of a host-form net_eval_pair call as a contiguous uint8 array [rows]: ValueError for another
    length, for more than 2^20 rows and for a value other than 0 (net_a) or 1 (net_b)."""
    side = np.asarray(side)
    if side.dtype == np.bool_:
        side = side.astype(np.uint8)
    if side.ndim != 1 or len(side) != rows:
        raise ValueError(f"net_eval_pair: side has shape {side.shape} for {rows} rows")
    if rows > ARENA_MAX_ROWS:
        raise ValueError(f"net_eval_pair: rows = {rows} must be 1 .. {ARENA_MAX_ROWS}")
    if not np.issubdtype(side.dtype, np.integer) or not ((side == 0) | (side == 1)).all():
        raise ValueError("net_eval_pair: side must be 0 (net_a) or 1 (net_b) in every row")
    return np.ascontiguousarray(side, dtype=np.uint8)


def check_selfplay_plies(plies: Any) -> int:
    """The `plies` of a selfplay_run call after its check: ValueError for anything but an integer >= 1."""
    if isinstance(plies, bool) or int(plies) != plies or not 1 <= int(plies) < 2**31:
        raise ValueError(f"selfplay_run: plies = {plies} must be at least 1")
    return int(plies)


def check_gumbel_batch_rows(logits: Any, values: Any, k: int, batch: int,
                            actions: int) -> tuple[np.ndarray, np.ndarray]:
    """The rows of a host-form gumbel_advance of a batch session, given with the slot axis ([k, B, A] and [k, B]) or
    flattened ([k B, A] and [k B]), as contiguous float32 arrays [k B, A] and [k B] after the checks of
    check_gumbel_rows."""
    with np.errstate(over="ignore"):
        logits = np.ascontiguousarray(logits, dtype=np.float32)
    if logits.shape not in ((k, batch, actions), (k * batch, actions)):
        raise ValueError(f"gumbel_advance: logits of shape {logits.shape} for a session of [{k}, {batch}, {actions}]")
    values = np.ascontiguousarray(values, dtype=np.float32)
    if values.shape not in ((k, batch), (k * batch,)):
        raise ValueError(f"gumbel_advance: values of shape {values.shape} for a session of [{k}, {batch}]")
    return check_gumbel_rows(logits.reshape(k * batch, actions), values.reshape(-1), k * batch, actions)


def device_count() -> int:
    n = ctypes.c_int32(0)
    check(lib().epa_device_count(ctypes.byref(n)))
    return n.value


def make_config(
    num_envs: int,
    batch_size: int = 0,
    seed: int = 42,
    env_seed: Sequence[int] | None = None,
    max_episode_steps: int = 0,
    device: int = 0,
    env_id_offset: int = 0,
    params: dict[str, float] | None = None,
) -> tuple[EpaConfig, list]:
    """Build an epa_config; returns (config, keepalive objects)."""
    keep: list = []
    cfg = EpaConfig()
    cfg.num_envs = num_envs
    cfg.batch_size = batch_size
    cfg.seed = seed
    if env_seed is not None and len(env_seed) > 0:
        arr = (ctypes.c_int32 * len(env_seed))(*[int(s) for s in env_seed])
        keep.append(arr)
        cfg.env_seed = ctypes.cast(arr, ctypes.POINTER(ctypes.c_int32))
    cfg.max_episode_steps = int(min(max_episode_steps, 2**31 - 1))
    cfg.device = device
    cfg.env_id_offset = env_id_offset
    params = params or {}
    cfg.n_params = len(params)
    if params:
        keys = (ctypes.c_char_p * len(params))(*[k.encode() for k in params])
        vals = (ctypes.c_double * len(params))(*[float(v) for v in params.values()])
        keep += [keys, vals]
        cfg.param_keys = ctypes.cast(keys, ctypes.POINTER(ctypes.c_char_p))
        cfg.param_values = ctypes.cast(vals, ctypes.POINTER(ctypes.c_double))
    return cfg, keep


def pool_keys(handle: ctypes.c_void_p, which: str = "state"):
    """[(name, np dtype, row shape tuple)] of an existing pool's state or action keys."""
    keys = (EpaKeyInfo * 32)()
    n = ctypes.c_int32(0)
    fn = lib().epa_pool_state_keys if which == "state" else lib().epa_pool_action_keys
    check(fn(handle, keys, 32, ctypes.byref(n)))
    return [(keys[i].name.decode(), DTYPES[keys[i].dtype], tuple(keys[i].shape[: keys[i].ndim]))
            for i in range(n.value)]


def describe(family: str, params: dict[str, float] | None = None, which: str = "state"):
    """[(name, np dtype, row shape tuple)] of a family's state or action keys."""
    cfg, keep = make_config(1, params=params)
    keys = (EpaKeyInfo * 32)()
    n = ctypes.c_int32(0)
    fn = lib().epa_describe_state if which == "state" else lib().epa_describe_action
    check(fn(family.encode(), ctypes.byref(cfg), keys, 32, ctypes.byref(n)))
    out = []
    for i in range(n.value):
        k = keys[i]
        out.append((k.name.decode(), DTYPES[k.dtype], tuple(k.shape[: k.ndim])))
    del keep
    return out


def family_players(family: str) -> int:
    """Players P of a family (1 for every single-player family)."""
    p = ctypes.c_int32(0)
    check(lib().epa_family_players(family.encode(), ctypes.byref(p)))
    return p.value


def describe_state_players(family: str, params: dict[str, float] | None = None) -> list[int]:
    """Per state key: P if its rows carry the leading player dimension ([k, P, ...] per batch), 1 otherwise."""
    cfg, keep = make_config(1, params=params)
    out = (ctypes.c_int32 * 32)()
    n = ctypes.c_int32(0)
    check(lib().epa_describe_state_players(family.encode(), ctypes.byref(cfg), out, 32, ctypes.byref(n)))
    del keep
    return [int(out[i]) for i in range(n.value)]
