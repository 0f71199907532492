"""NAMLUserEncoder / NRMSUserEncoder / LSTURUserEncoder / CAUMUserEncoder / MINSUserEncoder — mirror of reference
manner/models/components/user_encoder.py:9-89, 92-178, 181-243 (NAML: imported by the reference as ``UserEncoder``, cr_module.py:16;
NRMS: the user encoder of the PLM baselines; LSTUR, CAUM and MINS: opt-in, ``install(baselines=("lstur_plm",))`` / ``("caum_plm",)`` /
``("mins_plm",)``)."""
import torch
import torch.nn as nn

from manner_amd import hip, train
from manner_amd.models.components.attention import AdditiveAttention, DenseAttention, _differentiable


class NAMLUserEncoder(nn.Module):
    def __init__(self, news_embedding_dim: int, query_vector_dim: int) -> None:
        super().__init__()
        self.additive_attention = AdditiveAttention(input_dim=news_embedding_dim, query_dim=query_vector_dim)

    def forward(self, clicked_news_vector: torch.Tensor) -> torch.Tensor:
        # batch_size, num_clicked_news_per_user, news_embedding_dim -> batch_size, news_embedding_dim
        return self.additive_attention(clicked_news_vector)


class NRMSUserEncoder(nn.Module):
    """reference user_encoder.py:24-42.  Batch-faithful: the un-masked batch_first=False MultiheadAttention sees the dense
    [B, Hmax, D] history and so attends ACROSS THE USERS OF THE BATCH at each history slot (zero-padded slots included);
    the additive pooler then runs over all Hmax slots.  With grad mode on and anything that requires grad (train() or eval():
    the module has no dropout) the differentiable operators of manner_amd.train run — in-projection, axis-0 attention,
    out-projection and pooler, each with its hand-written backward (csrc/train_small.hip) — as
    baselines/nrms_plm_module.py:119-135 trains it; otherwise the inference kernels."""

    def __init__(self, news_embedding_dim: int, num_attention_heads: int, query_vector_dim: int) -> None:
        super().__init__()
        self.multihead_attention = nn.MultiheadAttention(news_embedding_dim, num_attention_heads)
        self.additive_attention = AdditiveAttention(news_embedding_dim, query_vector_dim)

    def forward(self, clicked_news_vector: torch.Tensor) -> torch.Tensor:
        mha = self.multihead_attention
        if torch.is_grad_enabled() and (clicked_news_vector.requires_grad or any(p.requires_grad for p in self.parameters())):
            if mha.dropout != 0.0:
                raise RuntimeError("attention-probability dropout inside nn.MultiheadAttention is not built (the reference uses 0)")
            user_vector = train.mha_axis0(clicked_news_vector, mha.in_proj_weight, mha.in_proj_bias, mha.out_proj.weight, mha.out_proj.bias,
                                          mha.num_heads)
            return self.additive_attention(user_vector)
        user_vector = hip.mha_axis0(clicked_news_vector, mha.in_proj_weight.detach(), mha.in_proj_bias.detach(),
                                    mha.out_proj.weight.detach(), mha.out_proj.bias.detach(), mha.num_heads)
        return self.additive_attention(user_vector)


class LSTURUserEncoder(nn.Module):
    """reference user_encoder.py:45-89 — LSTUR's long- and short-term user encoder (``install(baselines=("lstur_plm",))`` binds it):
    ``forward(user [B], clicked_news_vector [B, S, I], hist_size [B])`` returns every user's GRU state after its own ``hist_size[b]``
    steps — what the reference gets from ``pack_padded_sequence(enforce_sorted=False)`` and ``last_hidden`` — started from the user's
    embedding row (``ini`` -> [B, I]) or from zero with the row appended (``con`` -> [B, 2 (I // 2)]).

    One call is the gather of the user rows, the input projection and one launch per history slot (csrc/gru.hip); ``hist_size`` is read
    on the device, never copied to the host, and slots past it are never read.  The parameters live in an ``nn.Embedding`` and an
    ``nn.GRU`` of the reference's shapes, so the state-dict keys are the reference's; neither module's own forward runs.
    ``nn.Dropout2d`` on the [1, B, E] rows masks WHOLE USERS in train() (one draw per user and call, scaled by 1 / (1 - p)); the mirror
    does the same from one seed per call off torch's CPU generator, without torch's warning about the 3-D input.  Row 0 of the table is
    ``padding_idx``: it receives no gradient.  f32 whatever the autocast state.  A length outside [1, S] or a user id outside the table
    raises at the next ``hip.check_status()`` / status poll, as the other mirrors' input errors do."""

    def __init__(self, num_users: int, input_dim: int, user_masking_probability: float, long_short_term_method: str) -> None:
        super().__init__()
        assert long_short_term_method in ["ini", "con"]
        self.long_short_term_method = long_short_term_method
        hidden = input_dim if long_short_term_method == "ini" else int(input_dim * 0.5)
        self.long_term_user_embedding = nn.Embedding(num_embeddings=num_users, embedding_dim=hidden, padding_idx=0)
        self.dropout = nn.Dropout2d(p=user_masking_probability)
        self.gru = nn.GRU(input_dim, hidden)

    def _params(self):
        g = self.gru
        return [self.long_term_user_embedding.weight, g.weight_ih_l0, g.weight_hh_l0, g.bias_ih_l0, g.bias_hh_l0]

    def forward(self, user: torch.Tensor, clicked_news_vector: torch.Tensor, hist_size: torch.Tensor) -> torch.Tensor:
        dev = clicked_news_vector.device
        hip.status_poll(dev)
        p = self.dropout.p if self.training else 0.0
        if p > 0.0 or _differentiable(self, clicked_news_vector):
            seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if p > 0.0 else 0
            out = train.lstur_user(user, clicked_news_vector, hist_size, self._params(), self.long_short_term_method, p=p, seed=seed)
        else:
            out = hip.lstur_user(user, clicked_news_vector, hist_size, [t.detach() for t in self._params()], self.long_short_term_method)
        hip.status_arm(dev)
        return out


class CAUMUserEncoder(nn.Module):
    """reference user_encoder.py:92-178 — CAUM's candidate-aware user encoder (``install(baselines=("caum_plm",))`` binds it): called
    once per candidate column with the clicked news [B, S, D] and one candidate per user [B, D] (the strided ``cand[:, i, :]`` view of
    baselines/caum_plm_module.py, read in place), it returns the B scores.

    One call is one library entry (csrc/caum.hip): the window operand [x[s-1], x[s], x[s+1], c] (circular) and [c, x[s]] are packed
    by a kernel, never by torch; the attention runs at head dim 25 (the reference's 400 / 16) with the threads filled at small B; the
    candidate half of the dense attention's first Linear is computed once per user.  Batch-faithful to the reference: its
    nn.MultiheadAttention is batch_first=False but receives [B, S, U], so attention runs ACROSS THE B USERS OF THE CALL at each
    history slot, and the softmax over the history is unmasked (zero-padded slots take part).  ``DenseAttention(input_dim=2 U)`` is fed
    cat[all (U), candidate (D)]: as in the reference only D == U can run; construction stays legal, ``forward`` refuses D != U.
    f32 whatever the autocast state.  The three dropouts are on in train() only and draw one seed per call from torch's CPU generator
    (sites 7, 8, 9 of the counter-based generator).  ``forward_all`` takes the whole dense candidate tensor [B, C, D]: at evaluation
    time it is one library call for all C columns, otherwise the reference's loop over ``forward`` — or, with ``train_all_columns`` set,
    one training call for all columns."""

    #: opt-in: ``forward_all`` in train() (dropout on, or a graph recorded) as ONE ``train.caum_scores_all`` call over all columns
    #: instead of the loop over ``forward`` — the same seed draws and masks; sums in another order, so not the loop's bits
    train_all_columns = False

    def __init__(self, news_vector_dim: int, num_filters: int, dense_att_hidden_dim1: int, dense_att_hidden_dim2: int, user_vector_dim: int,
                 num_attention_heads: int, dropout_probability: float) -> None:
        super().__init__()
        self.dropout1 = nn.Dropout(p=dropout_probability)
        self.dropout2 = nn.Dropout(p=dropout_probability)
        self.dropout3 = nn.Dropout(p=dropout_probability)
        self.linear1 = nn.Linear(news_vector_dim * 4, num_filters)
        self.linear2 = nn.Linear(news_vector_dim * 2, user_vector_dim)
        self.linear3 = nn.Linear(num_filters + user_vector_dim, user_vector_dim)
        self.dense_att = DenseAttention(input_dim=user_vector_dim * 2, hidden_dim1=dense_att_hidden_dim1, hidden_dim2=dense_att_hidden_dim2)
        self.multihead_attention = nn.MultiheadAttention(user_vector_dim, num_attention_heads)

    def _params(self):
        mha, da = self.multihead_attention, self.dense_att
        return [self.linear1.weight, self.linear1.bias, self.linear2.weight, self.linear2.bias, mha.in_proj_weight, mha.in_proj_bias,
                mha.out_proj.weight, mha.out_proj.bias, self.linear3.weight, self.linear3.bias, da.linear.weight, da.linear.bias,
                da.linear2.weight, da.linear2.bias, da.linear3.weight, da.linear3.bias]

    def forward(self, clicked_news_vector: torch.Tensor, cand_news_vector: torch.Tensor) -> torch.Tensor:
        mha = self.multihead_attention
        if mha.dropout != 0.0:
            raise RuntimeError("attention-probability dropout inside nn.MultiheadAttention is not built (the reference uses 0)")
        probs = {self.dropout1.p, self.dropout2.p, self.dropout3.p}
        if len(probs) != 1:
            raise RuntimeError("CAUMUserEncoder: the three dropouts share one probability in the reference; differing ones are not built")
        p = self.dropout1.p if self.training else 0.0
        if p > 0.0 or _differentiable(self, clicked_news_vector, cand_news_vector):
            seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if p > 0.0 else 0
            return train.caum_user_scores(clicked_news_vector, cand_news_vector, self._params(), mha.num_heads, p=p, seed=seed)
        return hip.caum_user_scores(clicked_news_vector, cand_news_vector, [t.detach() for t in self._params()], mha.num_heads)

    def forward_all(self, clicked_news_vector: torch.Tensor, cand_news_vector: torch.Tensor) -> torch.Tensor:
        """The candidate loop of CAUMPLMModule.forward (baselines/caum_plm_module.py:156-163): clicked news [B, S, D] and the dense
        candidates [B, C, D] -> scores [B, C], column i what ``forward(clicked_news_vector, cand_news_vector[:, i, :])`` returns.
        Without dropout and with nothing to differentiate (eval() under no_grad / inference_mode, or frozen weights and inputs) it is
        one library call that takes every history-only and candidate-only product once (``hip.caum_scores_all``).  In train() with
        p > 0 the reference draws fresh masks of the clicked news per column, and a recorded graph needs the per-column backward:
        then it is that loop itself over ``forward`` — the same seed draws, bits and gradients as the loop written by hand.  With the
        class attribute ``train_all_columns`` set, that case is one ``train.caum_scores_all`` call instead: one seed per column drawn
        exactly as the loop draws them (the CPU generator ends in the same state, the masks are the same), the C columns as rows of
        one forward and one backward on the matrix cores."""
        p = self.dropout1.p if self.training else 0.0
        if self.train_all_columns and (p > 0.0 or _differentiable(self, clicked_news_vector, cand_news_vector)):
            mha = self.multihead_attention
            if mha.dropout != 0.0:
                raise RuntimeError("attention-probability dropout inside nn.MultiheadAttention is not built (the reference uses 0)")
            if len({self.dropout1.p, self.dropout2.p, self.dropout3.p}) != 1:
                raise RuntimeError("CAUMUserEncoder: the three dropouts share one probability in the reference; differing ones are not built")
            # the loop's own draws, one per column in column order (none at p == 0): the CPU generator ends where the loop leaves it
            seeds = [int(torch.randint(0, 2 ** 62, (1,)).item()) for _ in range(cand_news_vector.shape[1])] if p > 0.0 else None
            return train.caum_scores_all(clicked_news_vector, cand_news_vector, self._params(), mha.num_heads, p=p, seeds=seeds)
        if p > 0.0 or _differentiable(self, clicked_news_vector, cand_news_vector):
            scores = torch.zeros(cand_news_vector.shape[0], cand_news_vector.shape[1], device=cand_news_vector.device)
            scores = scores.transpose(1, 0)
            for i in range(cand_news_vector.shape[1]):
                scores[i, :] = self.forward(clicked_news_vector, cand_news_vector[:, i, :])
            return scores.transpose(1, 0)
        mha = self.multihead_attention
        if mha.dropout != 0.0:
            raise RuntimeError("attention-probability dropout inside nn.MultiheadAttention is not built (the reference uses 0)")
        if len({self.dropout1.p, self.dropout2.p, self.dropout3.p}) != 1:
            raise RuntimeError("CAUMUserEncoder: the three dropouts share one probability in the reference; differing ones are not built")
        return hip.caum_scores_all(clicked_news_vector, cand_news_vector, [t.detach() for t in self._params()], mha.num_heads)


class MINSUserEncoder(nn.Module):
    """reference user_encoder.py:181-243 — MINS's multi-channel GRU user encoder (``install(baselines=("mins_plm",))`` binds it):
    ``forward(clicked_news_vector [B, S, D], hist_size [B])`` -> [B, D].

    Batch-faithful to the reference: its nn.MultiheadAttention (heads = channels, head dim D / C: 128 as shipped) is batch_first=False
    but receives [B, S, D], so attention runs ACROSS THE B USERS OF THE CALL at each history slot, unmasked, zero-padded slots
    included — d clicked_news_vector is therefore not zero past a user's ``hist_size``.  ``torch.chunk`` then gives C contiguous
    channels of width D / C, every one through the SAME ``nn.GRU`` on ``pack_padded_sequence(hist_size, enforce_sorted=False)``;
    ``last_hidden`` of the channels is concatenated.  Here that is one input projection and ONE launch for the whole recurrence of all
    B C sequences (csrc/mins.hip: W_hh in registers, H <= 128); ``hist_size`` is read on the device, never copied to the host, and the
    GRU never reads a slot past it.  The final AdditiveAttention runs over a sequence of ONE slot: the identity, bit for bit — it is not
    run, and where a graph is recorded its three parameters receive exact-zero gradients, as the reference's do.

    The parameters live in the reference's submodules (``multi_channel_gru.*`` aliases the one ``gru``), so the state-dict keys are the
    reference's; none of their own forwards runs.  As in the reference only ``num_filters == news_embedding_dim`` can run: construction
    stays legal, ``forward`` refuses.  f32 whatever the autocast state.  S <= 256, D / C <= 128; a length outside [1, S] raises at the
    next ``hip.check_status()`` / status poll."""

    def __init__(self, news_embedding_dim: int, query_vector_dim: int, num_filters: int, num_gru_channels: int) -> None:
        super().__init__()
        self.num_gru_channels = num_gru_channels
        self.multihead_attention = nn.MultiheadAttention(embed_dim=news_embedding_dim, num_heads=num_gru_channels)
        self.additive_attention = AdditiveAttention(input_dim=news_embedding_dim, query_dim=query_vector_dim)
        assert num_filters % num_gru_channels == 0
        self.gru = nn.GRU(int(num_filters / num_gru_channels), int(num_filters / num_gru_channels))
        self.multi_channel_gru = nn.ModuleList([self.gru for _ in range(num_gru_channels)])

    def _params(self):
        mha, g = self.multihead_attention, self.gru
        return [mha.in_proj_weight, mha.in_proj_bias, mha.out_proj.weight, mha.out_proj.bias, g.weight_ih_l0, g.weight_hh_l0, g.bias_ih_l0, g.bias_hh_l0]

    def forward(self, clicked_news_vector: torch.Tensor, hist_size: torch.Tensor) -> torch.Tensor:
        if self.multihead_attention.dropout != 0.0:
            raise RuntimeError("attention-probability dropout inside nn.MultiheadAttention is not built (the reference uses 0)")
        hip.mins_check_widths(clicked_news_vector.shape[-1], self.num_gru_channels * self.gru.input_size, self.num_gru_channels)
        dev = clicked_news_vector.device
        hip.status_poll(dev)
        if _differentiable(self, clicked_news_vector):
            pool = self.additive_attention
            out = train.mins_user(clicked_news_vector, hist_size, self._params(), self.num_gru_channels,
                                  pool=[pool.query, pool.linear.weight, pool.linear.bias])
        else:
            out = hip.mins_user(clicked_news_vector, hist_size, [t.detach() for t in self._params()], self.num_gru_channels)
        hip.status_arm(dev)
        return out
