"""AdditiveAttention, PolyAttention, TargetAwareAttention, DenseAttention — mirrors of reference
manner/models/components/attention.py:6-29, 32-84, 87-116, 119-141 (PolyAttention and TargetAwareAttention are MINER's,
``install(baselines=("miner",))`` binds them; DenseAttention is CAUM's, ``install(baselines=("caum_plm",))``)."""
from typing import Optional

import torch
import torch.nn as nn

from manner_amd import hip, train


class AdditiveAttention(nn.Module):
    def __init__(self, input_dim: int, query_dim: int) -> None:
        super().__init__()
        self.linear = nn.Linear(input_dim, query_dim)
        self.query = nn.Parameter(torch.empty(query_dim).uniform_(-0.1, 0.1))

    def forward(self, input_vector: torch.Tensor) -> torch.Tensor:
        """(batch, seq, dim) -> (batch, dim); unmasked softmax over ``seq`` as in the reference."""
        # autograd records this forward whenever the reference's torch ops would (train() or eval(): there is no dropout here)
        if torch.is_grad_enabled() and (input_vector.requires_grad or any(p.requires_grad for p in self.parameters())):
            return train.additive_pool(input_vector, self.linear.weight, self.linear.bias, self.query)      # with its backward
        return hip.additive_pool(input_vector, self.linear.weight.detach(), self.linear.bias.detach(),
                                 self.query.detach())


def _differentiable(module: nn.Module, *inputs: torch.Tensor) -> bool:
    """The rule of AdditiveAttention.forward: autograd records the forward whenever the reference's torch ops would."""
    return torch.is_grad_enabled() and (any(t.requires_grad for t in inputs) or any(p.requires_grad for p in module.parameters()))


class PolyAttention(nn.Module):
    def __init__(self, input_embed_dim: int, num_context_codes: int, context_code_dim: int) -> None:
        super().__init__()
        self.linear = nn.Linear(in_features=input_embed_dim, out_features=context_code_dim, bias=False)
        self.context_codes = nn.Parameter(nn.init.xavier_uniform_(torch.empty(num_context_codes, context_code_dim),
                                                                  gain=nn.init.calculate_gain("tanh")))

    def forward(self, clicked_news_vector: torch.Tensor, attn_mask: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
        """(batch, hist, dim), (batch, hist) bool, (batch, hist, candidates of the batch) or None -> (batch, codes, dim); a masked slot
        keeps the logit 1e-30 and the bias mean runs over all its columns, as in the reference."""
        if _differentiable(self, clicked_news_vector):
            return train.poly_attention(clicked_news_vector, attn_mask, self.linear.weight, self.context_codes, bias)
        return hip.poly_attention(clicked_news_vector, attn_mask, self.linear.weight.detach(), self.context_codes.detach(),
                                  None if bias is None else bias.detach())


class DenseAttention(nn.Module):
    """reference attention.py:119-141 (CAUM's; ``install(baselines=("caum_plm",))`` binds it): Linear, tanh, Linear, tanh, Linear to one
    logit.  ``CAUMUserEncoder`` does not call this forward — its kernels read the parameters and split the first Linear between the
    history rows and the candidate — so this is the stand-alone operator, f32 whatever the autocast state."""

    def __init__(self, input_dim: int, hidden_dim1: int, hidden_dim2: int) -> None:
        super().__init__()
        self.linear = nn.Linear(input_dim, hidden_dim1)
        self.tanh1 = nn.Tanh()
        self.linear2 = nn.Linear(hidden_dim1, hidden_dim2)
        self.tanh2 = nn.Tanh()
        self.linear3 = nn.Linear(hidden_dim2, 1)

    def forward(self, input_vector: torch.Tensor) -> torch.Tensor:
        """(..., input_dim) -> (..., 1)"""
        l1, l2, l3 = self.linear, self.linear2, self.linear3
        if _differentiable(self, input_vector):
            t = train.linear_tanh(input_vector, l1.weight, l1.bias)
            t = train.linear_tanh(t, l2.weight, l2.bias)
            return train.linear(t, l3.weight, l3.bias)
        shape = input_vector.shape
        t = hip.linear_tanh(input_vector.reshape(-1, shape[-1]), l1.weight.detach(), l1.bias.detach())
        t = hip.linear_tanh(t, l2.weight.detach(), l2.bias.detach())
        return hip.linear(t, l3.weight.detach(), l3.bias.detach()).reshape(*shape[:-1], 1)


class TargetAwareAttention(nn.Module):
    def __init__(self, input_embed_dim: int) -> None:
        super().__init__()
        self.linear = nn.Linear(in_features=input_embed_dim, out_features=input_embed_dim, bias=False)

    def forward(self, query: torch.Tensor, key: torch.Tensor, value: torch.Tensor) -> torch.Tensor:
        """(batch, codes, dim), (batch, candidates, dim), (batch, candidates, codes) -> (batch, candidates)"""
        if _differentiable(self, query, key, value):
            return train.target_attention(query, key, value, self.linear.weight)
        return hip.target_attention(query, key, value, self.linear.weight.detach())
