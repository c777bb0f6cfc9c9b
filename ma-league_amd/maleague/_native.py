"""ctypes binding of libmaleague.so, the C ABI declared in include/maleague.h.

The HIP library is the product path: every op of the hot path calls into it. There is no CPU
fallback -- if the library is missing or no GPU is present, calls raise loudly.
Tensors cross the boundary as raw device pointers (``tensor.data_ptr()``) plus sizes; kernels run
on the caller's current HIP stream (``torch.cuda.current_stream().cuda_stream``).
"""
from __future__ import annotations

import ctypes
import os

import torch

MAXU = 64
_LIB_PATH = os.environ.get("MLG_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "_lib",
                                                      "libmaleague.so")


class NativeError(RuntimeError):
    """Raised when a libmaleague call fails (the C side's mlg_last_error())."""


class MlgEnvSpec(ctypes.Structure):
    _fields_ = [("U", ctypes.c_int32), ("n_agents", ctypes.c_int32), ("n_actions", ctypes.c_int32),
                ("grid", ctypes.c_int32), ("episode_limit", ctypes.c_int32), ("stochastic", ctypes.c_int32),
                ("policy_team", ctypes.c_int32), ("n_policy_teams", ctypes.c_int32),
                ("team", ctypes.c_int32 * MAXU), ("role", ctypes.c_int32 * MAXU), ("melee", ctypes.c_int32 * MAXU),
                ("agent_unit", ctypes.c_int32 * MAXU), ("scripted", ctypes.c_int32 * 2), ("seed", ctypes.c_uint64)]


class MlgEnvState(ctypes.Structure):
    _fields_ = [("x", ctypes.c_void_p), ("y", ctypes.c_void_p), ("hp", ctypes.c_void_p), ("t", ctypes.c_void_p),
                ("episode", ctypes.c_void_p), ("B", ctypes.c_int32)]


class MlgBatch(ctypes.Structure):
    _fields_ = [("state", ctypes.c_void_p), ("obs", ctypes.c_void_p), ("actions", ctypes.c_void_p),
                ("avail", ctypes.c_void_p), ("reward", ctypes.c_void_p), ("terminated", ctypes.c_void_p),
                ("actions_onehot", ctypes.c_void_p), ("filled", ctypes.c_void_p), ("B", ctypes.c_int32),
                ("T1", ctypes.c_int32), ("ring_slot0", ctypes.c_int32), ("ring_size", ctypes.c_int32),
                ("full_write", ctypes.c_int32), ("rows", ctypes.c_void_p), ("slot_extent", ctypes.c_void_p)]


class MlgRunInfo(ctypes.Structure):
    _fields_ = [("ep_len", ctypes.c_void_p), ("ret", ctypes.c_void_p), ("won", ctypes.c_void_p),
                ("draw", ctypes.c_void_p), ("agent_rows", ctypes.c_void_p), ("ret_away", ctypes.c_void_p)]


class MlgAgentParams(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in ["fc1_w", "fc1_b", "w_ih", "b_ih", "w_hh", "b_hh", "fc2_w", "fc2_b"]]


class MlgAgentDims(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ["d_obs", "n_actions", "n_agents", "hidden", "d_in", "obs_last_action",
                                              "obs_agent_id"]]


class MlgFFParams(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in ["fc1_w", "fc1_b", "fc2_w", "fc2_b"]]


class MlgQMixParams(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in ["hw1_0w", "hw1_0b", "hw1_2w", "hw1_2b", "hwf_0w", "hwf_0b", "hwf_2w",
                                              "hwf_2b", "hb1_w", "hb1_b", "v0_w", "v0_b", "v2_w", "v2_b"]] + \
               [(n, ctypes.c_int32) for n in ["n_agents", "state_dim", "embed_dim", "hypernet_embed",
                                              "hypernet_layers"]]


class MlgLearnerCfg(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ["B", "T", "N", "A", "d_obs", "H", "S", "E", "HE", "hypernet_layers",
                                              "mixer", "double_q", "obs_last_action", "obs_agent_id"]] + \
               [(n, ctypes.c_float) for n in ["gamma", "lr", "optim_alpha", "optim_eps", "grad_norm_clip"]] + \
               [("agent", ctypes.c_int32),  # 0 DRQN, 1 feed-forward (dqn)
                ("distinct", ctypes.c_int32),  # 1: one DRQN per agent slot (mac: distinct), vectors [agent 0 | .. | mixer]
                ("per", ctypes.c_int32)]  # 1: prioritized replay: the loss weights is_weight, the episode errors td_abs


class MlgLearnerBufs(ctypes.Structure):
    _fields_ = [("batch", MlgBatch)] + [(n, ctypes.c_void_p) for n in ["params", "grads", "square_avg",
                                                                      "target_params", "workspace", "stats",
                                                                      "target_sync", "trained_steps", "host_rows",
                                                                      "is_weight", "td_abs"]]


class MlgEntityEnvSpec(ctypes.Structure):
    _fields_ = [("base", MlgEnvSpec), ("min_agents", ctypes.c_int32), ("max_agents", ctypes.c_int32)]


class MlgEntityBatch(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in ["entities", "obs_mask", "entity_mask", "actions", "avail", "reward",
                                              "terminated", "actions_onehot", "filled"]] + \
               [(n, ctypes.c_int32) for n in ["B", "T1", "ring_slot0", "ring_size", "full_write"]] + \
               [("rows", ctypes.c_void_p), ("slot_extent", ctypes.c_void_p)]


class MlgRefilDims(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ["n_agents", "n_entities", "entity_shape", "n_actions",
                                              "entity_last_action", "attn_embed_dim", "attn_n_heads",
                                              "rnn_hidden_dim"]]



class MlgRefilLearnerCfg(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ["B", "T", "n_agents", "n_entities", "entity_shape", "n_actions",
                                              "entity_last_action", "attn_embed_dim", "attn_n_heads", "rnn_hidden_dim",
                                              "hypernet_embed", "mixing_embed_dim", "double_q",
                                              "softmax_mixing_weights", "imagine", "mixer"]] + \
               [(n, ctypes.c_float) for n in ["gamma", "lmbda", "lr", "optim_alpha", "optim_eps", "grad_norm_clip"]]


class MlgRefilLearnerBufs(ctypes.Structure):
    _fields_ = [("batch", MlgEntityBatch)] + [(n, ctypes.c_void_p) for n in ["groupA", "params", "grads", "square_avg",
                                                                           "target_params", "workspace", "stats",
                                                                           "trained_steps", "target_sync",
                                                                           "host_rows"]]


class MlgCrossplayPair(ctypes.Structure):
    _fields_ = [("home", ctypes.c_int32), ("away", ctypes.c_int32), ("spec", ctypes.c_int32)]


class MlgCrossplay(ctypes.Structure):
    _fields_ = [("packed_pool", ctypes.c_void_p), ("n_pool", ctypes.c_int32), ("n_pairs", ctypes.c_int32),
                ("pairs", ctypes.c_void_p), ("host_pairs", ctypes.c_void_p), ("specs", ctypes.c_void_p),
                ("host_specs", ctypes.c_void_p), ("n_specs", ctypes.c_int32), ("E", ctypes.c_int32),
                ("episode0", ctypes.c_uint32), ("workspace", ctypes.c_void_p), ("workspace_floats", ctypes.c_int64),
                ("ep_len", ctypes.c_void_p), ("ret", ctypes.c_void_p), ("ret_away", ctypes.c_void_p),
                ("won", ctypes.c_void_p), ("draw", ctypes.c_void_p), ("summary", ctypes.c_void_p)]


class MlgMixGroup(ctypes.Structure):
    _fields_ = [("away", ctypes.c_int32), ("spec", ctypes.c_int32)]


class MlgOpponentMix(ctypes.Structure):
    _fields_ = [("packed_pool", ctypes.c_void_p), ("n_pool", ctypes.c_int32), ("n_groups", ctypes.c_int32),
                ("groups", ctypes.c_void_p), ("host_groups", ctypes.c_void_p), ("specs", ctypes.c_void_p),
                ("host_specs", ctypes.c_void_p), ("n_specs", ctypes.c_int32)]


class MlgComaCfg(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ["B", "T", "N", "A", "d_obs", "S", "hidden"]] + \
               [(n, ctypes.c_float) for n in ["lr", "optim_eps", "grad_norm_clip"]] + \
               [(n, ctypes.c_double) for n in ["gamma", "td_lambda", "optim_alpha"]]


class MlgComaBufs(ctypes.Structure):
    _fields_ = [("batch", MlgBatch)] + [(n, ctypes.c_void_p) for n in ["params", "grads", "square_avg",
                                                                      "target_params", "workspace", "q_vals",
                                                                      "targets", "stats", "counters"]]


_P = ctypes.c_void_p
_I = ctypes.c_int32
# name -> (restype, argtypes); mirrors include/maleague.h one for one.
SIGNATURES = {
    "mlg_packed_agent_size": (ctypes.c_int64, [_P]),
    "mlg_pack_agent": (ctypes.c_int, [_P, _P, _P, _P]),
    "mlg_env_reset": (ctypes.c_int, [_P, _P, _P]),
    "mlg_env_step": (ctypes.c_int, [_P, _P, _P, _P, _P, _P, _P, _P]),
    "mlg_env_observe": (ctypes.c_int, [_P, _P, _P, _P, _P, _P]),
    "mlg_rollout": (ctypes.c_int, [_P, _P, _P, _P, _P, _P, ctypes.c_float, _I, _P]),
    "mlg_rollout_selfplay": (ctypes.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, ctypes.c_float, ctypes.c_float, _I, _P]),
    "mlg_rollout_describe": (ctypes.c_int, [_P, _P, _I, _P, _I, _P]),
    "mlg_agent_forward": (ctypes.c_int, [_P, _P, _P, _P, _P, _P, _I, _P]),
    "mlg_mac_forward": (ctypes.c_int, [_P, _P, _P, _I, _P, _P, _P, _P]),
    "mlg_select_actions": (ctypes.c_int, [_P, _P, _I, _I, _I, _P, _P, _I, ctypes.c_float, _P, _P, _P]),
    "mlg_qmix_forward": (ctypes.c_int, [_P, _P, _P, _P, _I, _P]),
    "mlg_agent_backward_workspace_floats": (ctypes.c_int64, [_P, _I]),
    "mlg_agent_backward": (ctypes.c_int, [_P] * 11 + [_I, _P]),
    "mlg_qmix_backward_workspace_floats": (ctypes.c_int64, [_P, _I]),
    "mlg_qmix_backward": (ctypes.c_int, [_P] * 7 + [_I, _P]),
    "mlg_qlearner_param_counts": (ctypes.c_int64, [_P, _P, _P]),
    "mlg_qlearner_workspace_floats": (ctypes.c_int64, [_P]),
    "mlg_qlearner_inline_rows": (ctypes.c_int, []),
    "mlg_qlearner_train": (ctypes.c_int, [_P, _P, _P]),
    "mlg_qlearner_describe": (ctypes.c_int, [_P, _P, _I]),
    "mlg_zero_slots_bytes": (ctypes.c_int, [_P, _P, _I, _I, _I, _P]),
    "mlg_refil_packed_agent_size": (ctypes.c_int64, [_P]),
    "mlg_refil_pack_agent": (ctypes.c_int, [_P, _P, _P, _P]),
    "mlg_refil_agent_forward": (ctypes.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _I, _P]),
    "mlg_refil_rollout": (ctypes.c_int, [_P, _P, _P, _P, _P, _P, ctypes.c_float, _I, _P]),
    "mlg_refil_rollout_describe": (ctypes.c_int, [_P, _P, _P, _I, _P]),
    "mlg_refil_rollout_selfplay": (ctypes.c_int, [_P] * 8 + [ctypes.c_float, ctypes.c_float, _I, _P]),
    "mlg_refil_rollout_selfplay_describe": (ctypes.c_int, [_P, _P, _P, _I, _P]),
    "mlg_refil_attention": (ctypes.c_int, [_P] * 6 + [_I] * 4 + [_P] * 2),
    "mlg_refil_packed_mixer_size": (ctypes.c_int64, [_P]),
    "mlg_refil_pack_mixer": (ctypes.c_int, [_P, _P, _P, _P]),
    "mlg_refil_mixer_forward": (ctypes.c_int, [_P] * 7 + [_I, _P, _I, _P]),
    "mlg_refil_attention_backward_workspace_floats": (ctypes.c_int64, [_I] * 4),
    "mlg_refil_attention_backward": (ctypes.c_int, [_P] * 7 + [_I] * 4 + [_P] * 4),
    "mlg_refil_mixer_backward_workspace_floats": (ctypes.c_int64, [_P, _I, _I]),
    "mlg_refil_mixer_backward": (ctypes.c_int, [_P] * 7 + [_I] + [_P] * 4 + [_I, _P]),
    "mlg_refil_agent_backward_workspace_floats":(ctypes.c_int64, [_P, _I]),
    "mlg_refil_agent_backward": (ctypes.c_int, [_P] * 11 + [_I, _P]),
    "mlg_refil_param_counts": (ctypes.c_int64, [_P, _P, _P]),
    "mlg_refil_workspace_floats": (ctypes.c_int64, [_P]),
    "mlg_refil_train": (ctypes.c_int, [_P, _P, _P]),
    "mlg_debug_set_stamps": (ctypes.c_int, [_P]),
    "mlg_debug_set_learner_stamps": (ctypes.c_int, [_P]),
    "mlg_refil_debug_set_stamps": (ctypes.c_int, [_P]),
    "mlg_league_record_runs": (ctypes.c_int, [_P, _P, _I, _P, _I, _P]),
    "mlg_refil_draw_groups": (ctypes.c_int, [_I, _I, ctypes.c_uint64, ctypes.c_uint32, _P, _P]),
    "mlg_crossplay_workspace_floats": (ctypes.c_int64, [_P, _I, _I]),
    "mlg_crossplay_rollout": (ctypes.c_int, [_P, _P, _P]),
    "mlg_pack_agent_pool": (ctypes.c_int, [_P, _P, ctypes.c_int64, _I, _P, _P]),
    "mlg_policy_probs": (ctypes.c_int, [_P, _P, _I, _I, ctypes.c_float, _I, _I, _P, _P]),
    "mlg_policy_probs_backward": (ctypes.c_int, [_P, _P, _P, _I, _I, ctypes.c_float, _I, _I, _P, _P]),
    "mlg_select_multinomial": (ctypes.c_int, [_P, _P, _I, _I, _I, _P, _P, _I, _I, _P, _P]),
    "mlg_rollout_policy": (ctypes.c_int, [_P, _P, _P, _P, _P, _P, ctypes.c_float, _I, _I, _I, _P]),
    "mlg_rollout_policy_describe": (ctypes.c_int, [_P, _P, _P, _I, _P]),
    "mlg_rollout_selfplay_policy": (ctypes.c_int, [_P] * 8 + [ctypes.c_float, ctypes.c_float, _I, _I, _I, _P]),
    "mlg_rollout_selfplay_policy_describe": (ctypes.c_int, [_P, _P, _P, _I, _P]),
    "mlg_crossplay_rollout_policy": (ctypes.c_int, [_P, _P, _I, _I, _P]),
    "mlg_coma_policy_loss": (ctypes.c_int, [_P, _P, _P, _P, _P, _I, _I, _I, _P, _P, _P]),
    "mlg_coma_param_count": (ctypes.c_int64, [_P]),
    "mlg_coma_workspace_floats": (ctypes.c_int64, [_P]),
    "mlg_coma_critic_train": (ctypes.c_int, [_P, _P, _P]),
    "mlg_coma_target_update": (ctypes.c_int, [_P, _P, ctypes.c_int64, _P, _I, _P]),
    "mlg_ff_packed_size": (ctypes.c_int64, [_P]),
    "mlg_ff_pack": (ctypes.c_int, [_P, _P, _P, _P]),
    "mlg_ff_forward": (ctypes.c_int, [_P, _P, _P, _P, _I, _P]),
    "mlg_ff_mac_forward": (ctypes.c_int, [_P, _P, _P, _I, _P, _P]),
    "mlg_ff_backward_workspace_floats": (ctypes.c_int64, [_P, _I]),
    "mlg_ff_backward": (ctypes.c_int, [_P] * 8 + [_I, _P]),
    "mlg_rollout_ff": (ctypes.c_int, [_P, _P, _P, _P, _P, _P, ctypes.c_float, _I, _P]),
    "mlg_rollout_ff_describe": (ctypes.c_int, [_P, _P, _P, _I, _P]),
    "mlg_ff_pack_pool": (ctypes.c_int, [_P, _P, ctypes.c_int64, _I, _P, _P]),
    "mlg_rollout_selfplay_ff": (ctypes.c_int, [_P] * 8 + [ctypes.c_float, ctypes.c_float, _I, _P]),
    "mlg_rollout_selfplay_ff_describe": (ctypes.c_int, [_P, _P, _P, _I, _P]),
    "mlg_crossplay_ff_workspace_floats": (ctypes.c_int64, [_P, _I, _I]),
    "mlg_crossplay_rollout_ff": (ctypes.c_int, [_P, _P, _P]),
    "mlg_mac_forward_distinct": (ctypes.c_int, [_P, _P, _P, _I, _P, _P, _P, _P]),
    "mlg_rollout_distinct": (ctypes.c_int, [_P, _P, _P, _P, _P, _P, ctypes.c_float, _I, _P]),
    "mlg_rollout_distinct_describe": (ctypes.c_int, [_P, _P, _P, _I, _P]),
    "mlg_rollout_selfplay_distinct": (ctypes.c_int, [_P] * 8 + [ctypes.c_float, ctypes.c_float, _I, _P]),
    "mlg_rollout_selfplay_distinct_describe": (ctypes.c_int, [_P, _P, _P, _I, _P]),
    "mlg_crossplay_rollout_distinct": (ctypes.c_int, [_P, _P, _P]),
    "mlg_rollout_selfplay_mix": (ctypes.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, ctypes.c_float, ctypes.c_float, _I, _P]),
    "mlg_rollout_selfplay_mix_describe": (ctypes.c_int, [_P, _P, _P, _I, _P]),
    "mlg_league_record_runs_mix": (ctypes.c_int, [_P, _P, _I, _P, _I, _P, ctypes.c_int64, _I, _P]),
    "mlg_per_lds_slots": (ctypes.c_int32, []),
    "mlg_per_max_slots": (ctypes.c_int32, []),
    "mlg_per_sample": (ctypes.c_int, [_P, _I, _I, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_double, _P, _P, _P,
                                      ctypes.c_int64, _P]),
    "mlg_per_insert": (ctypes.c_int, [_P, _I, _I, _I, _P, ctypes.c_double, ctypes.c_double, _P, _P]),
    "mlg_per_update": (ctypes.c_int, [_P, _I, _P, _P, _I, ctypes.c_double, ctypes.c_double, _P, _P]),
    "mlg_last_error": (ctypes.c_char_p, []),
    "mlg_version": (ctypes.c_char_p, []),
}

_lib = None


def lib_path() -> str:
    return _LIB_PATH


def load(require_gpu: bool = False):
    """Load libmaleague.so (raises if it has not been built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            raise NativeError(f"libmaleague.so not found at {_LIB_PATH}; build it with `make -C ma-league_amd` "
                              "(or __graft_entry__.build()). There is no CPU fallback.")
        lib = ctypes.CDLL(_LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    if require_gpu and not torch.cuda.is_available():
        raise NativeError("maleague kernels need a ROCm GPU (gfx950); torch.cuda.is_available() is False")
    return _lib


def call(name: str, *args) -> None:
    """Invoke a status-returning entry point; raise NativeError with mlg_last_error() on failure."""
    lib = load(require_gpu=True)
    rc = getattr(lib, name)(*args)
    if rc != 0:
        raise NativeError(f"{name} failed: {lib.mlg_last_error().decode()}")


def rollout_describe(spec: MlgEnvSpec, dims: MlgAgentDims, selfplay: bool = False) -> tuple[str, int]:
    """(kernel name, dynamic LDS bytes) of the launch mlg_rollout / mlg_rollout_selfplay would make for this spec
    and agent dims under the current MLG_ROLLOUT_* environment (mlg_rollout_describe: host only, needs no GPU)."""
    lib = load()
    name = ctypes.create_string_buffer(32)
    lds = ctypes.c_int64(0)
    rc = lib.mlg_rollout_describe(ctypes.byref(spec), ctypes.byref(dims), int(bool(selfplay)), name, len(name),
                                  ctypes.byref(lds))
    if rc != 0:
        raise NativeError(f"mlg_rollout_describe failed: {lib.mlg_last_error().decode()}")
    return name.value.decode(), int(lds.value)


def rollout_selfplay_mix_describe(spec: MlgEnvSpec, dims: MlgAgentDims) -> tuple[str, int]:
    """(arm name, dynamic LDS bytes) of the launch mlg_rollout_selfplay_mix would make for this shape under the current
    MLG_ROLLOUT_* environment: "sp8-mix" or "v1-mix/tpwK" (mlg_rollout_selfplay_mix_describe: host only)."""
    lib = load()
    name = ctypes.create_string_buffer(32)
    lds = ctypes.c_int64(0)
    rc = lib.mlg_rollout_selfplay_mix_describe(ctypes.byref(spec), ctypes.byref(dims), name, len(name),
                                               ctypes.byref(lds))
    if rc != 0:
        raise NativeError(f"mlg_rollout_selfplay_mix_describe failed: {lib.mlg_last_error().decode()}")
    return name.value.decode(), int(lds.value)


def rollout_policy_describe(spec: MlgEnvSpec, dims: MlgAgentDims) -> tuple[str, int]:
    """(instantiation name, dynamic LDS bytes) of the launch mlg_rollout_policy would make for this spec and agent
    dims (mlg_rollout_policy_describe: host only, needs no GPU)."""
    lib = load()
    name = ctypes.create_string_buffer(32)
    lds = ctypes.c_int64(0)
    rc = lib.mlg_rollout_policy_describe(ctypes.byref(spec), ctypes.byref(dims), name, len(name), ctypes.byref(lds))
    if rc != 0:
        raise NativeError(f"mlg_rollout_policy_describe failed: {lib.mlg_last_error().decode()}")
    return name.value.decode(), int(lds.value)


def rollout_selfplay_policy_describe(spec: MlgEnvSpec, dims: MlgAgentDims) -> tuple[str, int]:
    """(arm name, dynamic LDS bytes) of the launch mlg_rollout_selfplay_policy would make for this spec and one side's
    agent dims under the current MLG_ROLLOUT_GLOBAL_WEIGHTS environment: "sp-policy-lds/tpwK" or "sp-policy-global/tpwK"
    (mlg_rollout_selfplay_policy_describe: host only, needs no GPU)."""
    lib = load()
    name = ctypes.create_string_buffer(32)
    lds = ctypes.c_int64(0)
    rc = lib.mlg_rollout_selfplay_policy_describe(ctypes.byref(spec), ctypes.byref(dims), name, len(name),
                                                  ctypes.byref(lds))
    if rc != 0:
        raise NativeError(f"mlg_rollout_selfplay_policy_describe failed: {lib.mlg_last_error().decode()}")
    return name.value.decode(), int(lds.value)


def rollout_ff_describe(spec: MlgEnvSpec, dims: MlgAgentDims) -> tuple[str, int]:
    """(instantiation name, dynamic LDS bytes) of the launch mlg_rollout_ff would make for this spec and agent dims
    (mlg_rollout_ff_describe: host only, needs no GPU)."""
    lib = load()
    name = ctypes.create_string_buffer(32)
    lds = ctypes.c_int64(0)
    rc = lib.mlg_rollout_ff_describe(ctypes.byref(spec), ctypes.byref(dims), name, len(name), ctypes.byref(lds))
    if rc != 0:
        raise NativeError(f"mlg_rollout_ff_describe failed: {lib.mlg_last_error().decode()}")
    return name.value.decode(), int(lds.value)


def rollout_selfplay_ff_describe(spec: MlgEnvSpec, dims: MlgAgentDims) -> tuple[str, int]:
    """(arm name "ffsp-lds/tpwK" or "ffsp-global/tpwK", dynamic LDS bytes) of the launch mlg_rollout_selfplay_ff would
    make for this spec and one side's agent dims under the current MLG_ROLLOUT_GLOBAL_WEIGHTS environment
    (mlg_rollout_selfplay_ff_describe: host only, needs no GPU)."""
    lib = load()
    name = ctypes.create_string_buffer(32)
    lds = ctypes.c_int64(0)
    rc = lib.mlg_rollout_selfplay_ff_describe(ctypes.byref(spec), ctypes.byref(dims), name, len(name),
                                              ctypes.byref(lds))
    if rc != 0:
        raise NativeError(f"mlg_rollout_selfplay_ff_describe failed: {lib.mlg_last_error().decode()}")
    return name.value.decode(), int(lds.value)


def rollout_distinct_describe(spec: MlgEnvSpec, dims: MlgAgentDims) -> tuple[str, int]:
    """(instantiation name, dynamic LDS bytes) of the launch mlg_rollout_distinct would make for this spec and agent
    dims (mlg_rollout_distinct_describe: host only, needs no GPU)."""
    lib = load()
    name = ctypes.create_string_buffer(32)
    lds = ctypes.c_int64(0)
    rc = lib.mlg_rollout_distinct_describe(ctypes.byref(spec), ctypes.byref(dims), name, len(name), ctypes.byref(lds))
    if rc != 0:
        raise NativeError(f"mlg_rollout_distinct_describe failed: {lib.mlg_last_error().decode()}")
    return name.value.decode(), int(lds.value)


def rollout_selfplay_distinct_describe(spec: MlgEnvSpec, dims: MlgAgentDims) -> tuple[str, int]:
    """(arm name "dxsp-global/tpwK", dynamic LDS bytes) of the launch mlg_rollout_selfplay_distinct would make for this
    spec and one side's agent dims (mlg_rollout_selfplay_distinct_describe: host only, needs no GPU)."""
    lib = load()
    name = ctypes.create_string_buffer(32)
    lds = ctypes.c_int64(0)
    rc = lib.mlg_rollout_selfplay_distinct_describe(ctypes.byref(spec), ctypes.byref(dims), name, len(name),
                                                    ctypes.byref(lds))
    if rc != 0:
        raise NativeError(f"mlg_rollout_selfplay_distinct_describe failed: {lib.mlg_last_error().decode()}")
    return name.value.decode(), int(lds.value)


def refil_rollout_describe(spec: MlgEntityEnvSpec, dims: MlgRefilDims) -> tuple[str, int]:
    """(kernel name, dynamic LDS bytes) of the launch mlg_refil_rollout would make for this entity spec and agent dims
    under the current MLG_REFIL_ROLLOUT / MLG_REFIL_GENERIC environment (mlg_refil_rollout_describe: host only)."""
    lib = load()
    name = ctypes.create_string_buffer(32)
    lds = ctypes.c_int64(0)
    rc = lib.mlg_refil_rollout_describe(ctypes.byref(spec), ctypes.byref(dims), name, len(name), ctypes.byref(lds))
    if rc != 0:
        raise NativeError(f"mlg_refil_rollout_describe failed: {lib.mlg_last_error().decode()}")
    return name.value.decode(), int(lds.value)


def refil_rollout_selfplay_describe(spec: MlgEntityEnvSpec, dims: MlgRefilDims) -> tuple[str, int]:
    """(arm name "sp-ro2/kc1" | "sp-ro2/kc2" | "sp-ro2/kc3", dynamic LDS bytes) of the launch mlg_refil_rollout_selfplay
    would make for this two-policy entity spec and one side's agent dims (mlg_refil_rollout_selfplay_describe: host
    only, needs no GPU)."""
    lib = load()
    name = ctypes.create_string_buffer(32)
    lds = ctypes.c_int64(0)
    rc = lib.mlg_refil_rollout_selfplay_describe(ctypes.byref(spec), ctypes.byref(dims), name, len(name),
                                                 ctypes.byref(lds))
    if rc != 0:
        raise NativeError(f"mlg_refil_rollout_selfplay_describe failed: {lib.mlg_last_error().decode()}")
    return name.value.decode(), int(lds.value)


def qlearner_describe(cfg: MlgLearnerCfg) -> str:
    """"<agent part> + <mixer part>": the kernels mlg_qlearner_train would launch for this cfg under the current
    MLG_MIX_GENERIC environment (mlg_qlearner_describe: host only, needs no GPU; the names are in maleague.h)."""
    lib = load()
    name = ctypes.create_string_buffer(64)
    rc = lib.mlg_qlearner_describe(ctypes.byref(cfg), name, len(name))
    if rc != 0:
        raise NativeError(f"mlg_qlearner_describe failed: {lib.mlg_last_error().decode()}")
    return name.value.decode()


def stream_ptr(device=None) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def ptr(t: torch.Tensor | None) -> int | None:
    if t is None:
        return None
    if not t.is_cuda:
        raise NativeError(f"maleague kernels need device tensors, got a {t.device} tensor")
    if not t.is_contiguous():
        raise NativeError("maleague kernels need contiguous tensors")
    return t.data_ptr()


def byref(s):
    return ctypes.byref(s)
