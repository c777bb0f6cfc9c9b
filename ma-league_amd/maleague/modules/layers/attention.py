"""EntityAttentionLayer (API + state_dict keys of src/marl/modules/layers/attention.py:7-79).

Parameters and the ``scale_factor`` buffer are those of the reference (``in_trans.weight`` [3E, in],
``out_trans.weight`` [out, E], ``out_trans.bias``), so REFIL checkpoints interoperate. The computation runs
inside the REFIL kernels (refil_device.h attn_fwd / attn_bwd); ``forward`` calls mlg_refil_attention.
"""
from __future__ import annotations

import torch
import torch.nn as nn



class EntityAttentionLayer(nn.Module):
    def __init__(self, in_dim, embed_dim, out_dim, args):
        super().__init__()
        self.in_dim, self.embed_dim, self.out_dim = in_dim, embed_dim, out_dim
        self.n_heads = args.attn_n_heads
        self.n_agents = args.n_agents
        self.args = args
        assert self.embed_dim % self.n_heads == 0, "Embed dim must be divisible by n_heads"
        self.head_dim = self.embed_dim // self.n_heads
        dev = getattr(args, "device", "cpu")
        self.register_buffer("scale_factor", torch.scalar_tensor(self.head_dim, device=dev).sqrt())
        self.in_trans = nn.Linear(self.in_dim, self.embed_dim * 3, bias=False, device=dev)
        self.out_trans = nn.Linear(self.embed_dim, self.out_dim, device=dev)
        self._autograd = bool(getattr(args, "native_autograd", False))

    def enable_autograd(self, on: bool = True):
        """Opt in to a differentiable forward (also from ``args.native_autograd``): in grad mode, with a parameter or
        ``entities`` requiring grad, the parameters enter ``maleague::refil_attention`` live and ``loss.backward()``
        reaches them and ``entities`` (HIP backward, ``mlg_refil_attention_backward``). Off by default: forward
        then returns plain tensors as before. Values are bit-identical either way."""
        self._autograd = bool(on)
        return self

    def wants_grad(self, *tensors) -> bool:
        """The routing condition of the differentiable path."""
        return (getattr(self, "_autograd", False) and torch.is_grad_enabled()
                and (any(p.requires_grad for p in self.parameters())
                     or any(t is not None and t.requires_grad for t in tensors)))

    def forward(self, entities, pre_mask=None, post_mask=None, ret_attn_logits=None):
        """entities [bs, ne, in]; pre_mask [bs, >=nq, >=ne] (True/1 = masked); post_mask [bs, nq] -> [bs, nq, out]."""
        if ret_attn_logits is not None:
            raise NotImplementedError("ret_attn_logits is a diagnostic of the reference; not built")
        bs, ne, _ = entities.shape
        nq = post_mask.shape[1]
        dev = entities.device
        x = entities.float().contiguous()
        pre = pre_mask[:, :nq, :ne].to(torch.uint8).contiguous()
        post = post_mask.to(torch.uint8).contiguous()
        from ...ops import refil_attention
        if self.wants_grad(entities):
            return refil_attention(self.in_trans.weight.float().contiguous(), self.out_trans.weight.float().contiguous(),
                                   self.out_trans.bias.float().contiguous(), x, pre, post, int(self.n_heads))
        x = x.detach()
        w_in = self.in_trans.weight.detach().float().contiguous()
        w_out = self.out_trans.weight.detach().float().contiguous()
        b_out = self.out_trans.bias.detach().float().contiguous()
        return refil_attention(w_in, w_out, b_out, x, pre, post, int(self.n_heads))
