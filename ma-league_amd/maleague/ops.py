"""``torch.ops.maleague.*``: the stand-alone hot-path ops as PyTorch custom operators (the plugin
classes call the HIP library through ops PyTorch can see, next to the plain C ABI for non-torch callers).

Each op is registered with ``torch.library.custom_op`` (functional: it allocates its outputs) and a fake
(meta) implementation giving the output shapes, so ``torch.compile`` / graph capture treat it as one opaque node
instead of breaking the graph at a ctypes call. The implementation enqueues the ``libmaleague.so`` entry point
(include/maleague.h) on the current HIP stream of the inputs' device. There is no CPU implementation: the ops
raise on host tensors like every product path.

| op                                   | C ABI entry point         | reference                                           |
|--------------------------------------|---------------------------|-----------------------------------------------------|
| ``maleague::agent_forward``          | ``mlg_agent_forward``     | DRQNAgentNetwork.forward (drqn_agent.py:29-35)     |
| ``maleague::select_actions``         | ``mlg_select_actions``    | EpsilonGreedyActionSelector.select (action_selectors.py:44-62) |
| ``maleague::qmix_forward``           | ``mlg_qmix_forward``      | QMixer.forward (qmix.py:41-59)                      |
| ``maleague::refil_attention``        | ``mlg_refil_attention``   | EntityAttentionLayer.forward (attention.py:24-79)   |
| ``maleague::refil_mixer_forward``    | ``mlg_refil_mixer_forward`` | FlexQMixer.forward (flex_qmix.py:73-117)          |
| ``maleague::refil_agent_step``       | ``mlg_refil_agent_forward`` | EntityAttentionRNNAgent.forward, one step (entity_rnn_agent.py:32-65) |
| ``maleague::drqn_forward``           | ``mlg_agent_forward``     | DRQNAgentNetwork.forward with the live parameters as inputs (differentiable) |
| ``maleague::drqn_backward``          | ``mlg_agent_backward``    | its backward: one cell step (loss.backward(), q_learner.py:103) |
| ``maleague::ff_forward``             | ``mlg_ff_forward``        | DQNAgentNetwork.forward (dqn_agent.py:34-37): fc2(relu(fc1(inputs))) |
| ``maleague::dqn_forward``            | ``mlg_ff_forward``        | the same with the live parameters as inputs (differentiable) |
| ``maleague::dqn_backward``           | ``mlg_ff_backward``       | its backward w.r.t. the inputs and the parameters   |
| ``maleague::qmix_backward``          | ``mlg_qmix_backward``     | backward of ``qmix_forward`` w.r.t. agent_qs and the parameters |
| ``maleague::refil_attention_backward`` | ``mlg_refil_attention_backward`` | backward of ``refil_attention`` w.r.t. x and the parameters |
| ``maleague::flex_qmix_forward``      | ``mlg_refil_mixer_forward`` | FlexQMixer.forward with the live parameters as inputs (differentiable) |
| ``maleague::flex_qmix_backward``     | ``mlg_refil_mixer_backward`` | its backward w.r.t. agent_qs and the parameters (refil_learner.py:102-218) |
| ``maleague::entity_agent_forward``   | ``mlg_refil_agent_forward`` | EntityAttentionRNNAgent.forward, one step, with the live parameters as inputs (differentiable) |
| ``maleague::entity_agent_backward``  | ``mlg_refil_agent_backward`` | its backward w.r.t. h_in and the parameters |
| ``maleague::policy_probs``           | ``mlg_policy_probs``      | MultiAgentController._softmax (multi_agent_controller.py:78-99), differentiable |
| ``maleague::policy_probs_backward``  | ``mlg_policy_probs_backward`` | its backward w.r.t. the logits               |
| ``maleague::select_multinomial``     | ``mlg_select_multinomial`` | MultinomialActionSelector.select (action_selectors.py:11-32), counter RNG |
| ``maleague::coma_policy_loss``       | ``mlg_coma_policy_loss``  | the COMA actor loss (coma_learner.py:75-96), forward and d pi in one launch |

``drqn_forward``, ``dqn_forward``, ``qmix_forward``, ``refil_attention``, ``flex_qmix_forward`` and ``entity_agent_forward`` carry
autograd formulas (``torch.library.register_autograd``) that call the backward ops; the backward ops have none, so
double backward raises an error naming them. Gradients for ``packed``, ``dims``, the masks, the QMIX mixer's
``states`` and the REFIL ops' ``entities`` are ``None`` (states / entities that require grad are refused). The
modules route through the differentiable ops only after ``enable_autograd()``.

The rollout and learner entry points (``mlg_rollout*``, ``mlg_qlearner_train``, ``mlg_refil_train``) take the
replay ring, env state and optimizer state as in-place structs and stay direct calls of the stepper / learner
classes.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import torch
from torch import Tensor
from torch.library import custom_op, register_fake

from . import _native


def struct_fields(s) -> List[int]:
    """A ctypes dims struct (MlgAgentDims, MlgRefilDims, ...) as the int list the ops take."""
    return [int(getattr(s, f)) for f, _ in s._fields_]


def _stream(t: Tensor) -> int:
    return _native.stream_ptr(t.device)


def _opt(t: Optional[Tensor]):
    return None if t is None or t.numel() == 0 else _native.ptr(t)


# ---- DRQNAgentNetwork.forward ------------------------------------------------------------------------------
@custom_op("maleague::agent_forward", mutates_args=())
def agent_forward(packed: Tensor, inputs: Tensor, h_in: Tensor, dims: List[int]) -> Tuple[Tensor, Tensor]:
    """dims = [d_obs, n_actions, n_agents, hidden, d_in, obs_last_action, obs_agent_id] (MlgAgentDims);
    inputs [R, d_in], h_in [R, H] -> (q [R, A], h_out [R, H])."""
    d = _native.MlgAgentDims(*[int(v) for v in dims])
    R = inputs.shape[0]
    q = inputs.new_empty(R, d.n_actions)
    h_out = inputs.new_empty(R, d.hidden)
    _native.call("mlg_agent_forward", _native.byref(d), _native.ptr(packed), _native.ptr(inputs), _native.ptr(h_in),
                 _native.ptr(q), _native.ptr(h_out), R, _stream(inputs))
    return q, h_out


@register_fake("maleague::agent_forward")
def _agent_forward_fake(packed, inputs, h_in, dims):
    R = inputs.shape[0]
    return inputs.new_empty(R, dims[1]), inputs.new_empty(R, dims[3])


# ---- EpsilonGreedyActionSelector.select ----------------------------------------------------------------------
@custom_op("maleague::select_actions", mutates_args=())
def select_actions(q: Tensor, avail: Tensor, keys: Tensor, episodes: Tensor, t: int, epsilon: float
                   ) -> Tuple[Tensor, Tensor]:
    """q [B, N, A] f32, avail [B, N, A] int32, keys [B] int64 (counter-RNG key per env), episodes [B] int32 ->
    (actions [B, N] int64, is_greedy [B, N] int64)."""
    B, N, A = q.shape
    actions = torch.empty(B, N, dtype=torch.int64, device=q.device)
    greedy = torch.empty(B, N, dtype=torch.int64, device=q.device)
    _native.call("mlg_select_actions", _native.ptr(q), _native.ptr(avail), B * N, A, N, _native.ptr(keys),
                 _native.ptr(episodes), int(t), float(epsilon), _native.ptr(actions), _native.ptr(greedy), _stream(q))
    return actions, greedy


@register_fake("maleague::select_actions")
def _select_actions_fake(q, avail, keys, episodes, t, epsilon):
    B, N, _ = q.shape
    return q.new_empty(B, N, dtype=torch.int64), q.new_empty(B, N, dtype=torch.int64)


# ---- QMixer.forward ------------------------------------------------------------------------------------------
@custom_op("maleague::qmix_forward", mutates_args=())
def qmix_forward(params: List[Tensor], agent_qs: Tensor, states: Tensor, dims: List[int]) -> Tensor:
    """params = the 14 MlgQMixParams tensors in header order (zero-size for the absent second layers of a
    one-layer hypernet); dims = [n_agents, state_dim, embed_dim, hypernet_embed, hypernet_layers]; agent_qs [R, N],
    states [R, S] -> q_tot [R]."""
    p = _native.MlgQMixParams(*[_opt(t) for t in params], *[int(v) for v in dims])
    out = agent_qs.new_empty(agent_qs.shape[0])
    _native.call("mlg_qmix_forward", _native.byref(p), _native.ptr(agent_qs), _native.ptr(states), _native.ptr(out),
                 agent_qs.shape[0], _stream(agent_qs))
    return out


@register_fake("maleague::qmix_forward")
def _qmix_forward_fake(params, agent_qs, states, dims):
    return agent_qs.new_empty(agent_qs.shape[0])


# ---- EntityAttentionLayer.forward ----------------------------------------------------------------------------
@custom_op("maleague::refil_attention", mutates_args=())
def refil_attention(w_in: Tensor, w_out: Tensor, b_out: Tensor, x: Tensor, pre_mask: Tensor, post_mask: Tensor,
                    n_heads: int) -> Tensor:
    """x [bs, ne, in], pre_mask [bs, nq, ne] u8, post_mask [bs, nq] u8 -> y [bs, nq, out]."""
    bs, ne, _ = x.shape
    nq = post_mask.shape[1]
    y = x.new_empty(bs, nq, w_out.shape[0])
    _native.call("mlg_refil_attention", _native.ptr(w_in), _native.ptr(w_out), _native.ptr(b_out), _native.ptr(x),
                 _native.ptr(pre_mask), _native.ptr(post_mask), int(bs), int(ne), int(nq), int(n_heads),
                 _native.ptr(y), _stream(x))
    return y


@register_fake("maleague::refil_attention")
def _refil_attention_fake(w_in, w_out, b_out, x, pre_mask, post_mask, n_heads):
    return x.new_empty(x.shape[0], post_mask.shape[1], w_out.shape[0])


def _refil_dims(dims):
    return _native.MlgRefilDims(*[int(v) for v in dims])


# ---- FlexQMixer.forward --------------------------------------------------------------------------------------
@custom_op("maleague::refil_mixer_forward", mutates_args=())
def refil_mixer_forward(packed: Tensor, agent_qs: Tensor, entities: Tensor, entity_mask: Tensor,
                        w_mask: Optional[Tensor], i_mask: Optional[Tensor], softmax_mixing_weights: int,
                        dims: List[int]) -> Tensor:
    """dims = MlgRefilDims fields; agent_qs [R, NA] (or [R, 2 NA] with both imagine masks [R, NE, NE]),
    entities [R, NE, D0], entity_mask [R, NE] -> q_tot [R]."""
    d = _refil_dims(dims)
    R = agent_qs.shape[0]
    out = agent_qs.new_empty(R)
    _native.call("mlg_refil_mixer_forward", _native.byref(d), _native.ptr(packed), _native.ptr(agent_qs),
                 _native.ptr(entities), _native.ptr(entity_mask), _opt(w_mask), _opt(i_mask),
                 int(softmax_mixing_weights), _native.ptr(out), R, _stream(agent_qs))
    return out


@register_fake("maleague::refil_mixer_forward")
def _refil_mixer_forward_fake(packed, agent_qs, entities, entity_mask, w_mask, i_mask, softmax_mixing_weights, dims):
    return agent_qs.new_empty(agent_qs.shape[0])


# ---- EntityAttentionRNNAgent.forward, one step ---------------------------------------------------------------
@custom_op("maleague::refil_agent_step", mutates_args=())
def refil_agent_step(packed: Tensor, entities: Tensor, obs_mask: Tensor, entity_mask: Tensor, h_in: Tensor,
                     dims: List[int]) -> Tuple[Tensor, Tensor]:
    """entities [R, NE, D0], obs_mask [R, NE, NE] u8, entity_mask [R, NE] u8, h_in [R, NA, H] ->
    (q [R, NA, A], h_out [R, NA, H])."""
    d = _refil_dims(dims)
    R = entities.shape[0]
    q = entities.new_empty(R, d.n_agents, d.n_actions)
    h = entities.new_empty(R, d.n_agents, d.rnn_hidden_dim)
    _native.call("mlg_refil_agent_forward", _native.byref(d), _native.ptr(packed), _native.ptr(entities),
                 _native.ptr(obs_mask), _native.ptr(entity_mask), _native.ptr(h_in), _native.ptr(q), _native.ptr(h),
                 int(R), _stream(entities))
    return q, h


@register_fake("maleague::refil_agent_step")
def _refil_agent_step_fake(packed, entities, obs_mask, entity_mask, h_in, dims):
    R = entities.shape[0]
    return entities.new_empty(R, dims[0], dims[3]), entities.new_empty(R, dims[0], dims[7])


# ---- autograd: the agent step and the mixer call as differentiable ops ---------------------------------------
def _aligned(t: Optional[Tensor]) -> Optional[Tensor]:
    """Contiguous, on a 16-byte boundary (the kernels read rows of H floats as 16-byte vectors)."""
    if t is None:
        return None
    t = t.contiguous()
    return t.clone() if t.data_ptr() % 16 else t


def _workspace(name: str, like: Tensor, *args) -> Tensor:
    n = getattr(_native.load(require_gpu=True), name)(*args)
    if n < 0:
        raise _native.NativeError(f"{name} failed: {_native.load().mlg_last_error().decode()}")
    return like.new_empty(max(int(n), 4))


def _agent_numels(dims: List[int]) -> List[int]:
    """Sizes of the 8 agent parameters in named_parameters() order (AGENT_ORDER of learners/q_learner.py)."""
    A, H, d_in = dims[1], dims[3], dims[4]
    return [H * d_in, H, 3 * H * H, 3 * H * H, 3 * H, 3 * H, A * H, A]


@custom_op("maleague::drqn_forward", mutates_args=())
def drqn_forward(params: List[Tensor], packed: Tensor, inputs: Tensor, h_in: Tensor, dims: List[int]
                 ) -> Tuple[Tensor, Tensor]:
    """``agent_forward`` with the 8 live parameters (AGENT_ORDER: fc1.weight, fc1.bias, gru.weight_ih,
    gru.weight_hh, gru.bias_ih, gru.bias_hh, fc2.weight, fc2.bias) as inputs autograd can reach. The kernel reads
    ``packed``, which the caller guarantees is the pack of ``params``: values are bit-identical to ``agent_forward``."""
    d = _native.MlgAgentDims(*[int(v) for v in dims])
    R = inputs.shape[0]
    q = inputs.new_empty(R, d.n_actions)
    h_out = inputs.new_empty(R, d.hidden)
    _native.call("mlg_agent_forward", _native.byref(d), _native.ptr(packed), _native.ptr(inputs), _native.ptr(h_in),
                 _native.ptr(q), _native.ptr(h_out), R, _stream(inputs))
    return q, h_out


@register_fake("maleague::drqn_forward")
def _drqn_forward_fake(params, packed, inputs, h_in, dims):
    R = inputs.shape[0]
    return inputs.new_empty(R, dims[1]), inputs.new_empty(R, dims[3])


@custom_op("maleague::drqn_backward", mutates_args=())
def drqn_backward(params: List[Tensor], packed: Tensor, inputs: Tensor, h_in: Tensor, gq: Optional[Tensor],
                  gh_out: Optional[Tensor], dims: List[int]) -> Tuple[Tensor, Tensor, Tensor]:
    """Backward of one ``drqn_forward`` step (``mlg_agent_backward``): gq [R, A] / gh_out [R, H] (None = zero) ->
    (d_inputs [R, d_in], d_h_in [R, H], dflat: the 8 parameter gradients, flat, in AGENT_ORDER)."""
    d = _native.MlgAgentDims(*[int(v) for v in dims])
    R = inputs.shape[0]
    keep = [p.contiguous() for p in params]
    fc1w, fc1b, wih, whh, bih, bhh, fc2w, fc2b = [_native.ptr(p) for p in keep]
    cparams = _native.MlgAgentParams(fc1w, fc1b, wih, bih, whh, bhh, fc2w, fc2b)
    inputs, h_in = inputs.contiguous(), _aligned(h_in)
    gq = None if gq is None else gq.contiguous()
    gh_out = _aligned(gh_out)
    d_inputs = torch.empty_like(inputs)
    d_h_in = inputs.new_empty(R, d.hidden)
    dflat = inputs.new_empty(sum(_agent_numels(dims)))
    ws = _workspace("mlg_agent_backward_workspace_floats", inputs, _native.byref(d), R)
    _native.call("mlg_agent_backward", _native.byref(d), _native.byref(cparams), _native.ptr(packed),
                 _native.ptr(inputs), _native.ptr(h_in), _native.ptr(gq), _native.ptr(gh_out), _native.ptr(d_inputs),
                 _native.ptr(d_h_in), _native.ptr(dflat), _native.ptr(ws), R, _stream(inputs))
    return d_inputs, d_h_in, dflat


@register_fake("maleague::drqn_backward")
def _drqn_backward_fake(params, packed, inputs, h_in, gq, gh_out, dims):
    R = inputs.shape[0]
    return torch.empty_like(inputs), inputs.new_empty(R, dims[3]), inputs.new_empty(sum(_agent_numels(dims)))


def _split(dflat: Tensor, like: List[Tensor], needed) -> List[Optional[Tensor]]:
    """dflat as per-parameter views (zero-size entries -- absent layers -- and unneeded ones get None)."""
    out, off = [], 0
    for t, need in zip(like, needed):
        n = t.numel()
        out.append(dflat[off:off + n].view(t.shape) if need and n else None)
        off += n
    return out


def _drqn_setup(ctx, inputs, output):
    params, packed, x, h_in, dims = inputs
    ctx.set_materialize_grads(False)
    ctx.save_for_backward(*params, packed, x, h_in)
    ctx.dims = [int(v) for v in dims]


def _drqn_backward(ctx, gq, gh_out):
    *params, packed, x, h_in = ctx.saved_tensors
    if gq is None and gh_out is None:
        return [None] * len(params), None, None, None, None
    d_inputs, d_h_in, dflat = torch.ops.maleague.drqn_backward(list(params), packed, x, h_in, gq, gh_out, ctx.dims)
    need = ctx.needs_input_grad
    return (_split(dflat, list(params), need[0]), None, d_inputs if need[2] else None,
            d_h_in if need[3] else None, None)


torch.library.register_autograd("maleague::drqn_forward", _drqn_backward, setup_context=_drqn_setup)


# ---- DQNAgentNetwork.forward (feed-forward agent) ------------------------------------------------------------
def _ff_forward(packed: Tensor, inputs: Tensor, dims: List[int]) -> Tensor:
    d = _native.MlgAgentDims(*[int(v) for v in dims])
    R = inputs.shape[0]
    q = inputs.new_empty(R, d.n_actions)
    _native.call("mlg_ff_forward", _native.byref(d), _native.ptr(packed), _native.ptr(inputs), _native.ptr(q), R,
                 _stream(inputs))
    return q


@custom_op("maleague::ff_forward", mutates_args=())
def ff_forward(packed: Tensor, inputs: Tensor, dims: List[int]) -> Tensor:
    """dims = MlgAgentDims fields (hidden = the width of fc1); packed = the mlg_ff_pack() block;
    inputs [R, d_in] -> q [R, A] = fc2(relu(fc1(inputs)))."""
    return _ff_forward(packed, inputs, dims)


@register_fake("maleague::ff_forward")
def _ff_forward_fake(packed, inputs, dims):
    return inputs.new_empty(inputs.shape[0], dims[1])


def _ff_numels(dims: List[int]) -> List[int]:
    """Sizes of the 4 feed-forward agent parameters in named_parameters() order (DQNAgentNetwork.PARAM_ORDER)."""
    A, H, d_in = dims[1], dims[3], dims[4]
    return [H * d_in, H, A * H, A]


@custom_op("maleague::dqn_forward", mutates_args=())
def dqn_forward(params: List[Tensor], packed: Tensor, inputs: Tensor, dims: List[int]) -> Tensor:
    """``ff_forward`` with the 4 live parameters (fc1.weight, fc1.bias, fc2.weight, fc2.bias) as inputs autograd can
    reach. The kernel reads ``packed``, which the caller guarantees is the pack of ``params``: values are
    bit-identical to ``ff_forward``."""
    return _ff_forward(packed, inputs, dims)


@register_fake("maleague::dqn_forward")
def _dqn_forward_fake(params, packed, inputs, dims):
    return inputs.new_empty(inputs.shape[0], dims[1])


@custom_op("maleague::dqn_backward", mutates_args=())
def dqn_backward(params: List[Tensor], packed: Tensor, inputs: Tensor, gq: Optional[Tensor], dims: List[int]
                 ) -> Tuple[Tensor, Tensor]:
    """Backward of one ``dqn_forward`` call (``mlg_ff_backward``): gq [R, A] (None = zero) ->
    (d_inputs [R, d_in], dflat: the 4 parameter gradients, flat, in named_parameters() order)."""
    d = _native.MlgAgentDims(*[int(v) for v in dims])
    R = inputs.shape[0]
    keep = [p.contiguous() for p in params]
    cparams = _native.MlgFFParams(*[_native.ptr(p) for p in keep])
    inputs = inputs.contiguous()
    gq = None if gq is None else gq.contiguous()
    d_inputs = torch.empty_like(inputs)
    dflat = inputs.new_empty(sum(_ff_numels(dims)))
    ws = _workspace("mlg_ff_backward_workspace_floats", inputs, _native.byref(d), R)
    _native.call("mlg_ff_backward", _native.byref(d), _native.byref(cparams), _native.ptr(packed),
                 _native.ptr(inputs), _native.ptr(gq), _native.ptr(d_inputs), _native.ptr(dflat), _native.ptr(ws), R,
                 _stream(inputs))
    return d_inputs, dflat


@register_fake("maleague::dqn_backward")
def _dqn_backward_fake(params, packed, inputs, gq, dims):
    return torch.empty_like(inputs), inputs.new_empty(sum(_ff_numels(dims)))


def _dqn_setup(ctx, inputs, output):
    params, packed, x, dims = inputs
    ctx.set_materialize_grads(False)
    ctx.save_for_backward(*params, packed, x)
    ctx.dims = [int(v) for v in dims]


def _dqn_backward(ctx, gq):
    *params, packed, x = ctx.saved_tensors
    if gq is None:
        return [None] * len(params), None, None, None
    d_inputs, dflat = torch.ops.maleague.dqn_backward(list(params), packed, x, gq, ctx.dims)
    need = ctx.needs_input_grad
    return _split(dflat, list(params), need[0]), None, d_inputs if need[2] else None, None


torch.library.register_autograd("maleague::dqn_forward", _dqn_backward, setup_context=_dqn_setup)


@custom_op("maleague::qmix_backward", mutates_args=())
def qmix_backward(params: List[Tensor], agent_qs: Tensor, states: Tensor, g_qtot: Tensor, dims: List[int]
                  ) -> Tuple[Tensor, Tensor]:
    """Backward of ``qmix_forward`` (``mlg_qmix_backward``): g_qtot [R] -> (d_agent_qs [R, N], dflat: the gradients of
    the non-empty ``params`` in their order, flat). States get no gradient."""
    ps = [t.contiguous() for t in params]
    p = _native.MlgQMixParams(*[_opt(t) for t in ps], *[int(v) for v in dims])
    R = agent_qs.shape[0]
    agent_qs, states, g_qtot = agent_qs.contiguous(), states.contiguous(), g_qtot.contiguous()
    d_qs = torch.empty_like(agent_qs)
    dflat = agent_qs.new_empty(sum(t.numel() for t in ps))
    ws = _workspace("mlg_qmix_backward_workspace_floats", agent_qs, _native.byref(p), R)
    _native.call("mlg_qmix_backward", _native.byref(p), _native.ptr(agent_qs), _native.ptr(states),
                 _native.ptr(g_qtot), _native.ptr(d_qs), _native.ptr(dflat), _native.ptr(ws), R, _stream(agent_qs))
    return d_qs, dflat


@register_fake("maleague::qmix_backward")
def _qmix_backward_fake(params, agent_qs, states, g_qtot, dims):
    return torch.empty_like(agent_qs), agent_qs.new_empty(sum(t.numel() for t in params))


STATE_GRAD_ERROR = ("maleague::qmix_forward: gradients with respect to the states are not implemented "
                    "(pass states that do not require grad)")


def _qmix_setup(ctx, inputs, output):
    params, agent_qs, states, dims = inputs
    if states.requires_grad:
        raise _native.NativeError(STATE_GRAD_ERROR)
    ctx.save_for_backward(*params, agent_qs, states)
    ctx.dims = [int(v) for v in dims]


def _qmix_backward(ctx, g_qtot):
    *params, agent_qs, states = ctx.saved_tensors
    d_qs, dflat = torch.ops.maleague.qmix_backward(list(params), agent_qs, states, g_qtot, ctx.dims)
    need = ctx.needs_input_grad
    return _split(dflat, list(params), need[0]), d_qs if need[1] else None, None, None


torch.library.register_autograd("maleague::qmix_forward", _qmix_backward, setup_context=_qmix_setup)


# ---- autograd: the REFIL layer ops ------------------------------------------------------------------------------
ENTITY_GRAD_ERROR = ("maleague::{op}: gradients with respect to the entities are not implemented "
                     "(pass entities that do not require grad)")


@custom_op("maleague::refil_attention_backward", mutates_args=())
def refil_attention_backward(w_in: Tensor, w_out: Tensor, b_out: Tensor, x: Tensor, pre_mask: Tensor,
                             post_mask: Tensor, gy: Tensor, n_heads: int) -> Tuple[Tensor, Tensor]:
    """Backward of ``refil_attention`` (``mlg_refil_attention_backward``): gy [bs, nq, 64] -> (dx [bs, ne, 64], dflat:
    the gradients of in_trans.weight, out_trans.weight, out_trans.bias, flat)."""
    bs, ne, _ = x.shape
    nq = post_mask.shape[1]
    w_in, w_out, b_out = _aligned(w_in), _aligned(w_out), b_out.contiguous()
    x, gy = x.contiguous(), gy.contiguous()
    pre_mask, post_mask = pre_mask.contiguous(), post_mask.contiguous()
    dx = torch.empty_like(x)
    dflat = x.new_empty(w_in.numel() + w_out.numel() + b_out.numel())
    ws = _workspace("mlg_refil_attention_backward_workspace_floats", x, int(bs), int(ne), int(nq), int(n_heads))
    _native.call("mlg_refil_attention_backward", _native.ptr(w_in), _native.ptr(w_out), _native.ptr(b_out),
                 _native.ptr(x), _native.ptr(pre_mask), _native.ptr(post_mask), _native.ptr(gy), int(bs), int(ne),
                 int(nq), int(n_heads), _native.ptr(dx), _native.ptr(dflat), _native.ptr(ws), _stream(x))
    return dx, dflat


@register_fake("maleague::refil_attention_backward")
def _refil_attention_backward_fake(w_in, w_out, b_out, x, pre_mask, post_mask, gy, n_heads):
    return torch.empty_like(x), x.new_empty(w_in.numel() + w_out.numel() + b_out.numel())


def _attention_setup(ctx, inputs, output):
    w_in, w_out, b_out, x, pre_mask, post_mask, n_heads = inputs
    ctx.save_for_backward(w_in, w_out, b_out, x, pre_mask, post_mask)
    ctx.n_heads = int(n_heads)


def _attention_backward(ctx, gy):
    w_in, w_out, b_out, x, pre_mask, post_mask = ctx.saved_tensors
    dx, dflat = torch.ops.maleague.refil_attention_backward(w_in, w_out, b_out, x, pre_mask, post_mask, gy,
                                                            ctx.n_heads)
    need = ctx.needs_input_grad
    dw_in, dw_out, db_out = _split(dflat, [w_in, w_out, b_out], need[:3])
    return dw_in, dw_out, db_out, dx if need[3] else None, None, None, None


torch.library.register_autograd("maleague::refil_attention", _attention_backward, setup_context=_attention_setup)


@custom_op("maleague::flex_qmix_forward", mutates_args=())
def flex_qmix_forward(params: List[Tensor], packed: Tensor, agent_qs: Tensor, entities: Tensor, entity_mask: Tensor,
                      w_mask: Optional[Tensor], i_mask: Optional[Tensor], softmax_mixing_weights: int,
                      dims: List[int]) -> Tensor:
    """``refil_mixer_forward`` with the 28 live FlexQMixer parameters (named_parameters() order: hyper_w_1,
    hyper_w_final, hyper_b_1, V; each fc1.weight, fc1.bias, attn.in_trans.weight, attn.out_trans.weight,
    attn.out_trans.bias, fc2.weight, fc2.bias) as inputs autograd can reach. The kernel reads ``packed``, which the
    caller guarantees is the pack of ``params``: values are bit-identical to ``refil_mixer_forward``."""
    d = _refil_dims(dims)
    R = agent_qs.shape[0]
    out = agent_qs.new_empty(R)
    _native.call("mlg_refil_mixer_forward", _native.byref(d), _native.ptr(packed), _native.ptr(agent_qs),
                 _native.ptr(entities), _native.ptr(entity_mask), _opt(w_mask), _opt(i_mask),
                 int(softmax_mixing_weights), _native.ptr(out), R, _stream(agent_qs))
    return out


@register_fake("maleague::flex_qmix_forward")
def _flex_qmix_forward_fake(params, packed, agent_qs, entities, entity_mask, w_mask, i_mask, softmax_mixing_weights,
                            dims):
    return agent_qs.new_empty(agent_qs.shape[0])


@custom_op("maleague::flex_qmix_backward", mutates_args=())
def flex_qmix_backward(params: List[Tensor], packed: Tensor, agent_qs: Tensor, entities: Tensor, entity_mask: Tensor,
                       w_mask: Optional[Tensor], i_mask: Optional[Tensor], g_qtot: Tensor,
                       softmax_mixing_weights: int, dims: List[int]) -> Tuple[Tensor, Tensor]:
    """Backward of ``flex_qmix_forward`` (``mlg_refil_mixer_backward``): g_qtot [R] -> (d_agent_qs, the shape of
    agent_qs; dflat: the 28 parameter gradients, flat, in the order of ``params``). Entities and masks get none."""
    d = _refil_dims(dims)
    R = agent_qs.shape[0]
    agent_qs, entities, entity_mask = agent_qs.contiguous(), entities.contiguous(), entity_mask.contiguous()
    w_mask = None if w_mask is None else w_mask.contiguous()
    i_mask = None if i_mask is None else i_mask.contiguous()
    g_qtot = g_qtot.contiguous()
    d_qs = torch.empty_like(agent_qs)
    dflat = agent_qs.new_empty(sum(p.numel() for p in params))
    ws = _workspace("mlg_refil_mixer_backward_workspace_floats", agent_qs, _native.byref(d), R,
                    int(w_mask is not None))
    _native.call("mlg_refil_mixer_backward", _native.byref(d), _native.ptr(packed), _native.ptr(agent_qs),
                 _native.ptr(entities), _native.ptr(entity_mask), _native.ptr(w_mask), _native.ptr(i_mask),
                 int(softmax_mixing_weights), _native.ptr(g_qtot), _native.ptr(d_qs), _native.ptr(dflat),
                 _native.ptr(ws), R, _stream(agent_qs))
    return d_qs, dflat


@register_fake("maleague::flex_qmix_backward")
def _flex_qmix_backward_fake(params, packed, agent_qs, entities, entity_mask, w_mask, i_mask, g_qtot,
                             softmax_mixing_weights, dims):
    return torch.empty_like(agent_qs), agent_qs.new_empty(sum(p.numel() for p in params))


def _flex_qmix_setup(ctx, inputs, output):
    params, packed, agent_qs, entities, entity_mask, w_mask, i_mask, softmax, dims = inputs
    if entities.requires_grad:
        raise _native.NativeError(ENTITY_GRAD_ERROR.format(op="flex_qmix_forward"))
    ctx.imagine = w_mask is not None and i_mask is not None
    masks = [w_mask, i_mask] if ctx.imagine else []
    ctx.save_for_backward(*params, packed, agent_qs, entities, entity_mask, *masks)
    ctx.n_params = len(params)
    ctx.softmax = int(softmax)
    ctx.dims = [int(v) for v in dims]


def _flex_qmix_backward(ctx, g_qtot):
    saved = list(ctx.saved_tensors)
    params, (packed, agent_qs, entities, entity_mask), masks = (saved[:ctx.n_params],
                                                               saved[ctx.n_params:ctx.n_params + 4],
                                                               saved[ctx.n_params + 4:])
    w_mask, i_mask = masks if ctx.imagine else (None, None)
    d_qs, dflat = torch.ops.maleague.flex_qmix_backward(params, packed, agent_qs, entities, entity_mask, w_mask,
                                                        i_mask, g_qtot, ctx.softmax, ctx.dims)
    need = ctx.needs_input_grad
    return _split(dflat, params, need[0]), None, d_qs if need[2] else None, None, None, None, None, None, None


torch.library.register_autograd("maleague::flex_qmix_forward", _flex_qmix_backward, setup_context=_flex_qmix_setup)


@custom_op("maleague::entity_agent_forward", mutates_args=())
def entity_agent_forward(params: List[Tensor], packed: Tensor, entities: Tensor, obs_mask: Tensor,
                         entity_mask: Tensor, h_in: Tensor, dims: List[int]) -> Tuple[Tensor, Tensor]:
    """``refil_agent_step`` with the 13 live EntityAttentionRNNAgent parameters (named_parameters() order: fc1.weight,
    fc1.bias, attn.in_trans.weight, attn.out_trans.weight, attn.out_trans.bias, fc2.weight, fc2.bias,
    rnn.weight_ih, rnn.weight_hh, rnn.bias_ih, rnn.bias_hh, fc3.weight, fc3.bias) as inputs autograd can reach. The
    kernel reads ``packed``, which the caller guarantees is the pack of ``params``: values are bit-identical to
    ``refil_agent_step``."""
    d = _refil_dims(dims)
    R = entities.shape[0]
    q = entities.new_empty(R, d.n_agents, d.n_actions)
    h = entities.new_empty(R, d.n_agents, d.rnn_hidden_dim)
    _native.call("mlg_refil_agent_forward", _native.byref(d), _native.ptr(packed), _native.ptr(entities),
                 _native.ptr(obs_mask), _native.ptr(entity_mask), _native.ptr(h_in), _native.ptr(q), _native.ptr(h),
                 int(R), _stream(entities))
    return q, h


@register_fake("maleague::entity_agent_forward")
def _entity_agent_forward_fake(params, packed, entities, obs_mask, entity_mask, h_in, dims):
    R = entities.shape[0]
    return entities.new_empty(R, dims[0], dims[3]), entities.new_empty(R, dims[0], dims[7])


@custom_op("maleague::entity_agent_backward", mutates_args=())
def entity_agent_backward(params: List[Tensor], packed: Tensor, entities: Tensor, obs_mask: Tensor,
                          entity_mask: Tensor, h_in: Tensor, gq: Optional[Tensor], gh_out: Optional[Tensor],
                          dims: List[int]) -> Tuple[Tensor, Tensor]:
    """Backward of one ``entity_agent_forward`` step (``mlg_refil_agent_backward``): gq [R, NA, A] / gh_out
    [R, NA, H] (None = zero) -> (d_h_in [R, NA, H], dflat: the 13 parameter gradients, flat, in the order of
    ``params``). Entities and masks get none."""
    d = _refil_dims(dims)
    R = entities.shape[0]
    entities, obs_mask, entity_mask = entities.contiguous(), obs_mask.contiguous(), entity_mask.contiguous()
    h_in, gh_out = _aligned(h_in), _aligned(gh_out)
    gq = None if gq is None else gq.contiguous()
    d_h_in = entities.new_empty(R, d.n_agents, d.rnn_hidden_dim)
    dflat = entities.new_empty(sum(p.numel() for p in params))
    ws = _workspace("mlg_refil_agent_backward_workspace_floats", entities, _native.byref(d), R)
    _native.call("mlg_refil_agent_backward", _native.byref(d), _native.ptr(packed), _native.ptr(entities),
                 _native.ptr(obs_mask), _native.ptr(entity_mask), _native.ptr(h_in), _native.ptr(gq),
                 _native.ptr(gh_out), _native.ptr(d_h_in), _native.ptr(dflat), _native.ptr(ws), R, _stream(entities))
    return d_h_in, dflat


@register_fake("maleague::entity_agent_backward")
def _entity_agent_backward_fake(params, packed, entities, obs_mask, entity_mask, h_in, gq, gh_out, dims):
    return (entities.new_empty(entities.shape[0], dims[0], dims[7]),
            entities.new_empty(sum(p.numel() for p in params)))


def _entity_agent_setup(ctx, inputs, output):
    params, packed, entities, obs_mask, entity_mask, h_in, dims = inputs
    if entities.requires_grad:
        raise _native.NativeError(ENTITY_GRAD_ERROR.format(op="entity_agent_forward"))
    ctx.set_materialize_grads(False)
    ctx.save_for_backward(*params, packed, entities, obs_mask, entity_mask, h_in)
    ctx.dims = [int(v) for v in dims]


def _entity_agent_backward(ctx, gq, gh_out):
    *params, packed, entities, obs_mask, entity_mask, h_in = ctx.saved_tensors
    if gq is None and gh_out is None:
        return [None] * len(params), None, None, None, None, None, None
    d_h_in, dflat = torch.ops.maleague.entity_agent_backward(list(params), packed, entities, obs_mask, entity_mask,
                                                             h_in, gq, gh_out, ctx.dims)
    need = ctx.needs_input_grad
    return _split(dflat, list(params), need[0]), None, None, None, None, d_h_in if need[5] else None, None


torch.library.register_autograd("maleague::entity_agent_forward", _entity_agent_backward,
                                setup_context=_entity_agent_setup)


# ---- COMA: the policy output, multinomial selection and the actor loss -------------------------------------------
@custom_op("maleague::policy_probs", mutates_args=())
def policy_probs(logits: Tensor, avail: Tensor, epsilon: float, mask_before_softmax: int, test_mode: int) -> Tensor:
    """logits [..., A] f32, avail [..., A] int32 -> probabilities [..., A] (``mlg_policy_probs``)."""
    A = logits.shape[-1]
    x, av = logits.contiguous(), avail.contiguous()
    out = torch.empty_like(x)
    _native.call("mlg_policy_probs", _native.ptr(x), _native.ptr(av), x.numel() // A, A, float(epsilon),
                 int(mask_before_softmax), int(test_mode), _native.ptr(out), _stream(x))
    return out


@register_fake("maleague::policy_probs")
def _policy_probs_fake(logits, avail, epsilon, mask_before_softmax, test_mode):
    return torch.empty_like(logits, memory_format=torch.contiguous_format)


@custom_op("maleague::policy_probs_backward", mutates_args=())
def policy_probs_backward(logits: Tensor, avail: Tensor, g_probs: Tensor, epsilon: float, mask_before_softmax: int,
                          test_mode: int) -> Tensor:
    """Backward of ``policy_probs`` (``mlg_policy_probs_backward``): g_probs [..., A] -> d logits [..., A]."""
    A = logits.shape[-1]
    x, av, g = logits.contiguous(), avail.contiguous(), g_probs.contiguous()
    out = torch.empty_like(x)
    _native.call("mlg_policy_probs_backward", _native.ptr(x), _native.ptr(av), _native.ptr(g), x.numel() // A, A,
                 float(epsilon), int(mask_before_softmax), int(test_mode), _native.ptr(out), _stream(x))
    return out


@register_fake("maleague::policy_probs_backward")
def _policy_probs_backward_fake(logits, avail, g_probs, epsilon, mask_before_softmax, test_mode):
    return torch.empty_like(logits, memory_format=torch.contiguous_format)


def _policy_probs_setup(ctx, inputs, output):
    logits, avail, epsilon, mask, test_mode = inputs
    ctx.save_for_backward(logits, avail)
    ctx.cfg = (float(epsilon), int(mask), int(test_mode))


def _policy_probs_backward(ctx, g):
    logits, avail = ctx.saved_tensors
    return torch.ops.maleague.policy_probs_backward(logits, avail, g, *ctx.cfg), None, None, None, None


torch.library.register_autograd("maleague::policy_probs", _policy_probs_backward, setup_context=_policy_probs_setup)


@custom_op("maleague::select_multinomial", mutates_args=())
def select_multinomial(probs: Tensor, avail: Tensor, keys: Tensor, episodes: Tensor, t: int, greedy: int) -> Tensor:
    """probs [B, N, A] f32, avail [B, N, A] int32, keys [B] int64, episodes [B] int32 -> actions [B, N] int64
    (``mlg_select_multinomial``: the counter-RNG draw of DESIGN.md §3.7, purpose 5)."""
    B, N, A = probs.shape
    actions = torch.empty(B, N, dtype=torch.int64, device=probs.device)
    _native.call("mlg_select_multinomial", _native.ptr(probs.contiguous()), _native.ptr(avail.contiguous()), B * N, A,
                 N, _native.ptr(keys), _native.ptr(episodes), int(t), int(greedy), _native.ptr(actions),
                 _stream(probs))
    return actions


@register_fake("maleague::select_multinomial")
def _select_multinomial_fake(probs, avail, keys, episodes, t, greedy):
    return probs.new_empty(probs.shape[0], probs.shape[1], dtype=torch.int64)


@custom_op("maleague::coma_policy_loss", mutates_args=())
def coma_policy_loss(pi: Tensor, avail: Tensor, actions: Tensor, q_vals: Tensor, mask: Tensor
                     ) -> Tuple[Tensor, Tensor]:
    """The COMA actor loss (coma_learner.py:75-96; ``mlg_coma_policy_loss``): pi / avail (int32) / q_vals
    [B, T-1, N, A], actions [B, T-1, N, 1] int64, mask [B, T-1] or [B, T-1, 1] f32 -> (stats [4] = loss,
    advantage_mean, the masked mean of pi.max, the sum of the expanded mask; d loss / d pi [B, T-1, N, A])."""
    B, Tm, N, A = pi.shape
    p, av, q = pi.contiguous(), avail.contiguous(), q_vals.contiguous()
    ac, mk = actions.contiguous(), mask.contiguous()
    stats = p.new_empty(4)
    d_pi = torch.empty_like(p)
    _native.call("mlg_coma_policy_loss", _native.ptr(p), _native.ptr(av), _native.ptr(ac), _native.ptr(q),
                 _native.ptr(mk), B * Tm, N, A, _native.ptr(stats), _native.ptr(d_pi), _stream(p))
    return stats, d_pi


@register_fake("maleague::coma_policy_loss")
def _coma_policy_loss_fake(pi, avail, actions, q_vals, mask):
    return pi.new_empty(4), torch.empty_like(pi, memory_format=torch.contiguous_format)


def _coma_policy_loss_setup(ctx, inputs, output):
    ctx.set_materialize_grads(False)
    ctx.save_for_backward(output[1])


def _coma_policy_loss_backward(ctx, g_stats, g_dpi):
    (d_pi,) = ctx.saved_tensors
    # only the loss (stats[0]) depends on pi in the reference: the advantage is detached and the other entries are logs
    g = None if g_stats is None else g_stats[0] * d_pi
    return g, None, None, None, None


torch.library.register_autograd("maleague::coma_policy_loss", _coma_policy_loss_backward,
                                setup_context=_coma_policy_loss_setup)


OPS = ("agent_forward", "select_actions", "qmix_forward", "refil_attention", "refil_mixer_forward",
       "refil_agent_step", "drqn_forward", "drqn_backward", "qmix_backward", "refil_attention_backward",
       "flex_qmix_forward", "flex_qmix_backward", "entity_agent_forward", "entity_agent_backward",
       "policy_probs", "policy_probs_backward", "select_multinomial", "coma_policy_loss")
