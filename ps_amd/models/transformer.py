"""BERT-base and Llama-3 models for the BASELINE.json north-star configs (random init, no
checkpoints, no network).

Compact in-repo definitions (transformers is not needed on the hot path): parameter shapes
and counts match the published architectures -- BERT-base 110M (12 x 768, 12 heads, FFN
3072, vocab 30522), Llama-3-8B 8.03B (32 x 4096, 32 q / 8 kv heads, FFN 14336, vocab
128256, RoPE theta 500000).  BERT attention runs the fused MFMA kernels of
csrc/kernels/attention.hip (S <= 128) and attention_long.hip (128 < S <= 512; S % 32 == 0) (right-padded batches too: ``BertForMLM.forward(..., lengths=)``,
``mlm_batch(..., lengths=)``; or unpadded, the encoder on the valid tokens only: ``forward(..., seqs=)``,
``mlm_batch(..., lengths=, packed=True)``), Llama's causal GQA attention the flash kernel of flash_attn.hip
(packed rows too: ``LlamaForCausalLM.forward(..., doc_ids=)``, ``packed_lm_batch``);
everything is bf16 on the GPU with fp32 masters on the parameter-server shards.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.utils.checkpoint import checkpoint

from ..ops.dense import SplitKLinear
from ..ops.linear import PsLinear
from ..ops.transformer import (PackedSeqs, attention_causal_gqa, attention_qkv, cross_entropy,
                              doc_bounds as _doc_bounds, layer_norm_residual, pack_seqs, rms_norm, rope_split,
                              rope_table, swiglu)


# ------------------------------------------------------------------------------------ BERT
@dataclass
class BertConfig:
    vocab: int = 30522
    hidden: int = 768
    layers: int = 12
    heads: int = 12
    ffn: int = 3072
    max_pos: int = 512
    type_vocab: int = 2
    eps: float = 1e-12
    dropout: float = 0.1


class BertLayer(nn.Module):
    def __init__(self, c: BertConfig):
        super().__init__()
        self.c = c
        # split-K weight gradients (ops/dense.py SplitKLinear): 32K tokens into small dW
        self.qkv = SplitKLinear(c.hidden, 3 * c.hidden)
        self.proj = SplitKLinear(c.hidden, c.hidden)
        self.ln1 = nn.LayerNorm(c.hidden, eps=c.eps)
        self.fc1 = SplitKLinear(c.hidden, c.ffn)
        self.fc2 = SplitKLinear(c.ffn, c.hidden)
        self.ln2 = nn.LayerNorm(c.hidden, eps=c.eps)

    def forward(self, x, mask: Optional[torch.Tensor] = None, key_lengths: Optional[torch.Tensor] = None,
                seqs: Optional[PackedSeqs] = None):
        """``seqs`` (ops.transformer.pack_seqs): ``x`` is [T, hidden], the valid tokens only -- every GEMM and
        row kernel runs on T rows, attention reads sequence b at its offset."""
        p = self.c.dropout if self.training else 0.0
        # fused MFMA attention over the qkv projection for S <= 128 (one tile) and 128 < S <= 512 (chunked),
        # S % 32 == 0 (ops/transformer.py), SDPA else;
        # key_lengths [B] (a right-padded batch) stays on the fused kernel, an arbitrary mask does not
        # fork: x's residual gradient is added inside the qkv / fc1 data-gradient GEMM (ops/dense.py)
        qkv, xr = self.qkv.fork(x)
        a = attention_qkv(qkv, self.c.heads, p, mask, key_lengths, seqs)
        # post-LN epilogues: LN(x + dropout(sublayer)) as one fused HIP pass each way
        x = layer_norm_residual(xr, self.proj(a), self.ln1.weight, self.ln1.bias, self.c.eps, p, self.training)
        h, xr = self.fc1.fork(x)
        f = self.fc2(F.gelu(h))
        return layer_norm_residual(xr, f, self.ln2.weight, self.ln2.bias, self.c.eps, p, self.training)


class BertForMLM(nn.Module):
    """BERT-base with the masked-LM head (decoder tied to the word embeddings)."""

    def __init__(self, c: BertConfig = BertConfig()):
        super().__init__()
        self.c = c
        self.word = nn.Embedding(c.vocab, c.hidden)
        self.pos = nn.Embedding(c.max_pos, c.hidden)
        self.tok_type = nn.Embedding(c.type_vocab, c.hidden)
        self.ln = nn.LayerNorm(c.hidden, eps=c.eps)
        self.layers = nn.ModuleList(BertLayer(c) for _ in range(c.layers))
        self.head_dense = nn.Linear(c.hidden, c.hidden)
        self.head_ln = nn.LayerNorm(c.hidden, eps=c.eps)
        self.head_bias = nn.Parameter(torch.zeros(c.vocab))
        self.apply(self._init)

    @staticmethod
    def _init(m):
        if isinstance(m, (nn.Linear, nn.Embedding)):
            nn.init.normal_(m.weight, std=0.02)
        if isinstance(m, nn.Linear) and m.bias is not None:
            nn.init.zeros_(m.bias)

    def forward(self, ids, labels=None, positions=None, lengths=None, seqs: Optional[PackedSeqs] = None):
        """``positions`` [B, P] (the masked-LM positions of the original BERT pretraining input
        format, ``masked_lm_positions``): the LM head runs only on those B*P rows -- the vocab
        projection and its softmax are 1/(S/P) of the dense-head cost.  Without positions the
        head runs on every token (labels -100 are ignored).

        ``lengths`` [B] (any integer dtype): a right-padded batch -- tokens at or beyond
        ``lengths[b]`` of sequence b are padding that no token attends to (key lengths of every
        layer's attention); their labels should be -100 (``mlm_batch(..., lengths=)``).

        ``seqs`` (``pack_seqs(lengths, S)``, ``mlm_batch(..., lengths=, packed=True)``; not with
        ``lengths``): the same batch, unpadded -- ``ids`` / ``labels`` / ``positions`` keep their [B, S] /
        [B, P] format, but the embeddings, every layer and the head run on the T valid tokens only.  With
        ``positions`` the head rows are those positions (logits [B * P, V], as without ``seqs``); without
        them the head runs on the T tokens and, with no ``labels``, the logits come back as [T, V] in
        packed order (``ops.transformer.repad`` gives [B, S, V])."""
        if seqs is not None:
            if lengths is not None:
                raise ValueError("BertForMLM: give lengths (padded) or seqs (unpadded), not both")
            x, labels = self._encode_packed(ids, labels, positions, seqs)
            return self._head(x, labels)
        b, s = ids.shape
        pos = torch.arange(s, device=ids.device)
        x = self.word(ids) + self.pos(pos)[None] + self.tok_type.weight[0]
        x = F.dropout(self.ln(x), self.c.dropout, self.training)
        if lengths is None:
            for layer in self.layers:
                x = layer(x)
        else:  # converted once: every layer gets the int32 device tensor the kernel reads
            klen = torch.as_tensor(lengths).to(device=ids.device, dtype=torch.int32, non_blocking=True)
            for layer in self.layers:
                x = layer(x, key_lengths=klen)
        if positions is not None:
            flat = (positions + torch.arange(b, device=ids.device)[:, None] * s).reshape(-1)
            x = x.reshape(b * s, -1).index_select(0, flat)
            if labels is not None:
                labels = labels.reshape(-1).index_select(0, flat)
        return self._head(x, labels)

    def _head(self, x, labels):
        h = self.head_ln(F.gelu(self.head_dense(x)))
        logits = h @ self.word.weight.t() + self.head_bias
        if labels is None:
            return logits
        return cross_entropy(logits.view(-1, self.c.vocab), labels.reshape(-1), ignore_index=-100)

    def _encode_packed(self, ids, labels, positions, seqs: PackedSeqs):
        """The head's input rows and their labels from the T valid tokens of ``ids`` [B, S]."""
        b, s = ids.shape
        if (b, s) != (seqs.batch, seqs.seq):
            raise ValueError("BertForMLM: ids [seqs.batch, seqs.seq]")
        x = self.word(ids.reshape(-1).index_select(0, seqs.index)) + self.pos(seqs.pos) + self.tok_type.weight[0]
        x = F.dropout(self.ln(x), self.c.dropout, self.training)  # [T, hidden]
        for layer in self.layers:
            x = layer(x, seqs=seqs)
        if positions is not None:
            # row of position (b, p) in the packed order; the clamp only moves the filler of a sequence
            # masked in full, which mlm_batch points at a pad position (label -100)
            cu = seqs.cu.long()
            rows = (cu[:-1, None] + torch.minimum(positions, (cu[1:] - cu[:-1] - 1)[:, None])).reshape(-1)
            x = x.index_select(0, rows)
            if labels is not None:
                flat = (positions + torch.arange(b, device=ids.device)[:, None] * s).reshape(-1)
                labels = labels.reshape(-1).index_select(0, flat)
        elif labels is not None:
            labels = labels.reshape(-1).index_select(0, seqs.index)
        return x, labels


def _mlm_batch_padded(ids, g, mask_prob, lengths, device, with_positions, packed=False):
    """mlm_batch for a right-padded batch: ``ids`` are the full-length draws, ``g`` their generator."""
    batch, seq = ids.shape
    lens = torch.as_tensor(lengths, dtype=torch.int64).cpu()
    lens = lens.expand(batch).clone() if lens.dim() == 0 else lens
    if lens.shape != (batch,) or int(lens.min()) < 1 or int(lens.max()) > seq:
        raise ValueError("mlm_batch: lengths is an int or [batch] integers in [1, seq]")
    npred = torch.tensor([max(1, int(round(mask_prob * n))) for n in lens.tolist()])  # <= length
    cols = torch.arange(seq)[None, :]
    pad = cols >= lens[:, None]
    # a random order of each sequence's valid positions, its pad positions behind them
    order = torch.rand(batch, seq, generator=g).masked_fill(pad, 2.0).argsort(dim=1)
    P = int(npred.max())
    real = torch.arange(P)[None, :] < npred[:, None]  # [B, P]: a masked position, not a filler
    chosen = torch.zeros(batch, seq, dtype=torch.bool).scatter_(1, order[:, :P], real)
    # the filler: the next position of the order -- valid and unmasked, or (all of the sequence is
    # masked) a pad position; a row that needs a filler has npred < P <= seq, so the index exists
    filler = order.gather(1, npred.clamp(max=seq - 1)[:, None])
    positions = order[:, :P].masked_fill(~real, seq).sort(dim=1).values  # masked ones ascending, first
    positions = torch.where(positions < seq, positions, filler)
    labels = torch.where(chosen, ids, torch.full_like(ids, -100))
    ids = ids.masked_fill(chosen, 103).masked_fill(pad, 0)  # [MASK], [PAD]
    seqs = pack_seqs(lens, seq, device) if packed else None  # from the host lengths
    if device is not None:
        ids, labels, positions, lens = ids.to(device), labels.to(device), positions.to(device), lens.to(device)
    res = (ids, labels, positions, lens) if with_positions else (ids, labels, lens)
    return res + (seqs,) if packed else res


def mlm_batch(batch: int, seq: int, vocab: int = 30522, mask_prob: float = 0.15, seed: int = 0, device=None,
              with_positions: bool = False, lengths=None, packed: bool = False):
    """Synthetic MLM batch in the BERT pretraining format: exactly round(mask_prob * seq)
    masked positions per sequence (create_pretraining_data's num_to_predict), replaced by
    [MASK]; labels -100 elsewhere.  ``with_positions`` also returns masked_lm_positions [B, P].

    ``lengths`` (an int, or [batch] integers in [1, seq]) makes a right-padded batch and is returned
    last, as an int64 tensor: positions >= length hold id 0 ([PAD]) and label -100, and sequence b
    masks max(1, round(mask_prob * length_b)) positions of [0, length_b).  ``packed=True`` (with
    ``lengths``) appends the batch's ``PackedSeqs`` for ``BertForMLM.forward(..., seqs=)`` as one more,
    last, element.  ``positions`` stays
    rectangular at the batch maximum count: a shorter row is filled by repeating one of its valid
    unmasked positions (label -100, so the head ignores it; a sequence masked in full, such as one
    of length 1, repeats a pad position instead).  Without ``lengths`` the batch is what it always
    was for the seed."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(min(1000, vocab // 2), vocab, (batch, seq), generator=g)
    if packed and lengths is None:
        raise ValueError("mlm_batch: packed=True needs lengths")
    if lengths is not None:
        return _mlm_batch_padded(ids, g, mask_prob, lengths, device, with_positions, packed)
    npred = max(1, int(round(mask_prob * seq)))
    positions = torch.rand(batch, seq, generator=g).argsort(dim=1)[:, :npred].sort(dim=1).values
    labels = torch.full_like(ids, -100)
    labels.scatter_(1, positions, ids.gather(1, positions))
    ids = ids.scatter(1, positions, 103)  # [MASK]
    if device is not None:
        ids, labels, positions = ids.to(device), labels.to(device), positions.to(device)
    return (ids, labels, positions) if with_positions else (ids, labels)


# ----------------------------------------------------------------------------------- Llama
@dataclass
class LlamaConfig:
    vocab: int = 128256
    hidden: int = 4096
    layers: int = 32
    heads: int = 32
    kv_heads: int = 8
    ffn: int = 14336
    rope_theta: float = 500000.0
    eps: float = 1e-5
    max_seq: int = 8192

    @staticmethod
    def llama3_8b() -> "LlamaConfig":
        return LlamaConfig()

    @staticmethod
    def tiny() -> "LlamaConfig":
        return LlamaConfig(vocab=512, hidden=64, layers=2, heads=4, kv_heads=2, ffn=128, max_seq=128)


class RMSNorm(nn.Module):
    def __init__(self, d, eps):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(d))
        self.eps = eps

    def forward(self, x):
        return rms_norm(x, self.weight, self.eps)  # fused HIP kernel on GPU bf16 (ops/transformer.py)


class LlamaBlock(nn.Module):
    """Pre-norm decoder block.  Q/K/V and gate/up projections are single fused GEMMs
    (``wqkv`` [(H + 2 KV) * hd, D], ``w13`` [2 F, D] -- same parameter count as separate
    matrices, one hipBLASLt launch each); attention is the causal GQA flash kernel
    (csrc/kernels/flash_attn.hip; no K/V replication, output already head-merged)."""

    def __init__(self, c: LlamaConfig):
        super().__init__()
        self.c = c
        hd = c.hidden // c.heads
        self.attn_norm = RMSNorm(c.hidden, c.eps)
        # PsLinear: the weight gradient lands straight in the PS gradient bucket (ops/linear.py)
        self.wqkv = PsLinear(c.hidden, (c.heads + 2 * c.kv_heads) * hd, bias=False)
        self.wo = PsLinear(c.heads * hd, c.hidden, bias=False)
        self.mlp_norm = RMSNorm(c.hidden, c.eps)
        self.w13 = PsLinear(c.hidden, 2 * c.ffn, bias=False)
        self.w2 = PsLinear(c.ffn, c.hidden, bias=False)

    def forward(self, x, r, cs, doc_bounds=None):
        """Residual stream = x + r (r: the previous block's pending MLP output, None for the
        first block) -- the add is fused into this block's first RMSNorm, and this block's
        MLP output is returned pending for the next one.  ``doc_bounds`` (packed rows): the
        (doc_start, doc_end) pair of ops.transformer.doc_bounds, each token attends inside its document."""
        b, s, _ = x.shape
        c = self.c
        hd = c.hidden // c.heads
        if r is None:
            h = self.attn_norm(x)
        else:
            x, h = rms_norm(x, self.attn_norm.weight, c.eps, residual=r)
        qkv = self.wqkv(h).view(b, s, c.heads + 2 * c.kv_heads, hd)
        q, k, v = rope_split(qkv, cs, c.heads, c.kv_heads)  # RoPE + split + transpose, one pass
        o = self.wo(attention_causal_gqa(q, k, v, doc_bounds))  # flash kernel (heads merged) or SDPA
        x, h = rms_norm(x, self.mlp_norm.weight, c.eps, residual=o)
        return x, self.w2(swiglu(self.w13(h)))


class LlamaForCausalLM(nn.Module):
    def __init__(self, c: LlamaConfig = LlamaConfig(), checkpointing: bool = False):
        super().__init__()
        self.c = c
        self.checkpointing = checkpointing
        self.embed = nn.Embedding(c.vocab, c.hidden)
        self.layers = nn.ModuleList(LlamaBlock(c) for _ in range(c.layers))
        self.norm = RMSNorm(c.hidden, c.eps)
        self.lm_head = PsLinear(c.hidden, c.vocab, bias=False)
        for m in self.modules():
            if isinstance(m, (nn.Linear, nn.Embedding)):
                nn.init.normal_(m.weight, std=0.02)

    def forward(self, ids, labels=None, doc_ids=None):
        """``doc_ids`` [B, S] (any integer dtype): packed rows -- a new document begins wherever the id
        changes along a row, and a token attends only to earlier tokens of its own document (the bounds
        are computed once and given to every layer).  RoPE positions run on through the row: the
        scores depend on i - j alone, so inside a document they are those of restarted positions.  A
        position whose next token belongs to another document has no target."""
        s = ids.shape[1]
        cs = rope_table(s, self.c.hidden // self.c.heads, self.c.rope_theta, ids.device)
        bounds = None
        if doc_ids is not None:
            doc_ids = doc_ids.to(ids.device, non_blocking=True)
            if doc_ids.shape != ids.shape:
                raise ValueError("doc_ids: [B, S] like ids")
            bounds = _doc_bounds(doc_ids)
        x, r = self.embed(ids), None
        for layer in self.layers:
            if self.checkpointing and self.training:
                x, r = checkpoint(layer, x, r, cs, bounds, use_reentrant=False)
            else:
                x, r = layer(x, r, cs, bounds)
        _, h = rms_norm(x, self.norm.weight, self.c.eps, residual=r)
        logits = self.lm_head(h)
        if labels is None:
            return logits
        # next-token targets; the last position has none (ignored) -- no sliced copy of the logits
        tgt = torch.cat([labels[:, 1:], torch.full_like(labels[:, :1], -100)], dim=1)
        if doc_ids is not None:  # nor has a document's last position
            tgt[:, :-1].masked_fill_(doc_ids[:, 1:] != doc_ids[:, :-1], -100)
        return cross_entropy(logits, tgt, ignore_index=-100)


def packed_lm_batch(batch: int, seq: int, vocab: int, doc_lengths, seed: int = 0, device=None):
    """Synthetic packed causal-LM batch -> (ids, labels, doc_ids), each [batch, seq] int64:
    ``doc_lengths`` is one list of document lengths per row, each list summing to ``seq``
    (``ValueError`` otherwise); ``doc_ids`` numbers a row's documents 0, 1, ... and ``labels`` are the
    ids (``LlamaForCausalLM.forward(ids, labels, doc_ids)`` shifts them and drops the targets that
    would cross a document boundary)."""
    rows = [list(map(int, r)) for r in doc_lengths]
    if len(rows) != batch:
        raise ValueError("packed_lm_batch: one list of document lengths per row")
    for r in rows:
        if not r or min(r) < 1 or sum(r) != seq:
            raise ValueError("packed_lm_batch: every row's positive document lengths sum to seq")
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, vocab, (batch, seq), generator=g)
    doc_ids = torch.stack([torch.repeat_interleave(torch.arange(len(r)), torch.tensor(r)) for r in rows])
    labels = ids.clone()
    if device is not None:
        ids, labels, doc_ids = ids.to(device), labels.to(device), doc_ids.to(device)
    return ids, labels, doc_ids


def param_count(m: nn.Module) -> int:
    seen, n = set(), 0
    for p in m.parameters():
        if id(p) not in seen:
            seen.add(id(p))
            n += p.numel()
    return n
