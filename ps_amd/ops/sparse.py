"""Sparse-row ops for embedding / wide tables (HIP on GPU, torch on CPU).

``dedup_rows`` is the worker side of push_rows: it turns per-occurrence gradient rows into
(unique ids, reduced rows).  The sort/unique step uses torch (rocPRIM radix sort on the
GPU); the reduction itself is the deterministic ``segment_reduce_rows`` HIP kernel.
"""
from __future__ import annotations

import torch

from .. import knobs
from ._ext import native, use_native

ACT_NONE, ACT_RELU, ACT_LEAKY, ACT_SIGMOID = 0, 1, 2, 3


def _act_ref(x: torch.Tensor, act: int) -> torch.Tensor:
    if act == ACT_RELU:
        return torch.relu(x)
    if act == ACT_LEAKY:
        return torch.where(x > 0, x, 0.01 * x)
    if act == ACT_SIGMOID:
        return 0.001 + 0.998 * torch.sigmoid(x)
    return x


def gather_rows(table: torch.Tensor, rows: torch.Tensor, out: torch.Tensor | None = None, out_off: int = 0,
                act: int = ACT_NONE) -> torch.Tensor:
    """out[:, out_off:out_off+dim] = act(table[rows])."""
    dim = table.shape[1]
    if out is None:
        out = torch.empty(rows.numel(), dim, dtype=table.dtype, device=table.device)
    if use_native(table, rows):
        native().gather_rows(table, rows.contiguous(), out, int(out_off), int(act))
        return out
    out[:, out_off:out_off + dim] = _act_ref(table[rows].float(), act).to(out.dtype)
    return out


def segment_reduce_rows(src: torch.Tensor, perm: torch.Tensor, seg_off: torch.Tensor, out: torch.Tensor,
                        mean: bool = False) -> torch.Tensor:
    if use_native(src, perm):
        native().segment_reduce_rows(src, perm, seg_off, out, bool(mean))
        return out
    srt = src[perm].float()
    cnt = (seg_off[1:] - seg_off[:-1])
    seg_ids = torch.repeat_interleave(torch.arange(cnt.numel()), cnt)
    acc = torch.zeros(out.shape, dtype=torch.float32)
    acc.index_add_(0, seg_ids, srt)
    if mean:
        acc /= cnt.clamp(min=1).float()[:, None]
    out.copy_(acc.to(out.dtype))
    return out


def _bag_of(bag_off: torch.Tensor, nnz: int) -> torch.Tensor:
    """Bag index of every value position, from the bag offsets alone (no host sync)."""
    pos = torch.arange(nnz, dtype=torch.int64, device=bag_off.device)
    return torch.searchsorted(bag_off[1:].contiguous(), pos, right=True)


def _bag_scale(bag_off: torch.Tensor) -> torch.Tensor:
    """1 / max(1, len) per bag, fp32 (mean mode)."""
    return 1.0 / (bag_off[1:] - bag_off[:-1]).clamp(min=1).float()


def bag_pool_fwd(rows: torch.Tensor, inv: torch.Tensor, bag_off: torch.Tensor, out: torch.Tensor,
                 weights: torch.Tensor | None = None, mean: bool = False, return_path: bool = False):
    """out[g] = s_g * sum_{j in [bag_off[g], bag_off[g+1])} weights[j] * rows[inv[j]], s_g = 1 / max(1, len_g)
    in mean mode, else 1; an empty bag gives a zero row.  rows fp32 [nu, dim], out fp32 / bf16 [G, dim].

    GPU: the fused HIP kernel (csrc/kernels/bags.hip); with the ``bag_pool`` route disabled the
    composition of the one-hot kernels (gather_rows -> weight multiply -> segment_reduce_rows),
    which writes the [nnz, dim] rows to memory.  CPU: torch ops.  ``return_path`` -> (out, path):
    1 vector kernel, 0 generic kernel, -1 composition / CPU."""
    path = -1
    nnz = inv.numel()
    if use_native(rows, inv):
        if knobs.enabled("bag_pool"):
            path = int(native().bag_pool_fwd(rows, inv, bag_off, weights, out, bool(mean)))
        else:
            src = torch.empty(nnz, rows.shape[1], dtype=torch.float32, device=rows.device)
            native().gather_rows(rows, inv, src, 0, ACT_NONE)
            if weights is not None:
                src *= weights[:, None]
            pos = torch.arange(nnz, dtype=torch.int64, device=rows.device)
            native().segment_reduce_rows(src, pos, bag_off, out, bool(mean))
    else:
        src = rows[inv].float()
        if weights is not None:
            src = src * weights[:, None].float()
        acc = torch.zeros(out.shape, dtype=torch.float32).index_add_(0, _bag_of(bag_off, nnz), src)
        if mean:
            acc *= _bag_scale(bag_off)[:, None]
        out.copy_(acc.to(out.dtype))
    return (out, path) if return_path else out


def bag_pool_bwd(dout: torch.Tensor, perm: torch.Tensor, seg_off: torch.Tensor, bag_of: torch.Tensor,
                 bag_off: torch.Tensor, drows: torch.Tensor, weights: torch.Tensor | None = None,
                 mean: bool = False, return_path: bool = False):
    """drows[u] = sum_{j in [seg_off[u], seg_off[u+1])} weights[p] * s_{g} * dout[g], p = perm[j],
    g = bag_of[p]: the gradient of ``bag_pool_fwd`` w.r.t. the unique rows, summed per row in the
    sorted order of the plan (deterministic; an empty segment gives zeros).  dout fp32 / bf16
    [G, dim], drows fp32 [nseg, dim].  Paths as in ``bag_pool_fwd``."""
    path = -1
    if use_native(dout, perm):
        if knobs.enabled("bag_pool"):
            path = int(native().bag_pool_bwd(dout, perm, seg_off, bag_of, bag_off, weights, drows, bool(mean)))
        else:
            src = torch.empty(bag_of.numel(), dout.shape[1], dtype=torch.float32, device=dout.device)
            native().gather_rows(dout, bag_of, src, 0, ACT_NONE)
            scale = weights
            if mean:
                s = _bag_scale(bag_off)[bag_of]
                scale = s if scale is None else scale * s
            if scale is not None:
                src *= scale[:, None]
            native().segment_reduce_rows(src, perm, seg_off, drows, False)
    else:
        src = dout.float()[bag_of]
        scale = None if weights is None else weights.float()
        if mean:
            s = _bag_scale(bag_off)[bag_of]
            scale = s if scale is None else scale * s
        if scale is not None:
            src = src * scale[:, None]
        cnt = seg_off[1:] - seg_off[:-1]
        seg_ids = torch.repeat_interleave(torch.arange(cnt.numel()), cnt)
        acc = torch.zeros(drows.shape, dtype=torch.float32).index_add_(0, seg_ids, src[perm])
        drows.copy_(acc)
    return (drows, path) if return_path else drows


def dedup_rows(ids: torch.Tensor, grads: torch.Tensor, mean: bool = False, out_dtype=None):
    """(unique_ids, reduced_grads[u]) where reduced = sum (or mean) over occurrences."""
    ids = ids.reshape(-1)
    grads = grads.reshape(ids.numel(), -1)
    uniq, inverse, counts = torch.unique(ids, sorted=True, return_inverse=True, return_counts=True)
    perm = torch.argsort(inverse, stable=True)
    seg_off = torch.zeros(uniq.numel() + 1, dtype=torch.int64, device=ids.device)
    torch.cumsum(counts, 0, out=seg_off[1:])
    out = torch.empty(uniq.numel(), grads.shape[1], dtype=out_dtype or grads.dtype, device=grads.device)
    segment_reduce_rows(grads.contiguous(), perm, seg_off, out, mean)
    return uniq, out


def scatter_add_rows(src: torch.Tensor, rows: torch.Tensor, table: torch.Tensor) -> torch.Tensor:
    if use_native(src, table):
        native().scatter_add_rows(src.contiguous(), rows.contiguous(), table)
        return table
    table.index_add_(0, rows, src.float())
    return table


def embedding_bag_fwd(table: torch.Tensor, ids: torch.Tensor, out: torch.Tensor, out_off: int = 0,
                      act: int = ACT_NONE) -> torch.Tensor:
    """out[b, off + f*dim + d] = act(table[ids[b, f], d]) -- fused field lookup + concat."""
    if use_native(table, ids):
        native().embedding_bag_fwd(table, ids.contiguous(), out, int(out_off), int(act))
        return out
    b, f = ids.shape
    dim = table.shape[1]
    out[:, out_off:out_off + f * dim] = _act_ref(table[ids].reshape(b, f * dim), act).to(out.dtype)
    return out


def sparse_lr_fwd(w: torch.Tensor, ids: torch.Tensor, bias: torch.Tensor | None, out: torch.Tensor) -> torch.Tensor:
    """out[b] = sum_f w[ids[b,f] mod H] + bias (wide part)."""
    if use_native(w, ids):
        native().sparse_lr_fwd(w, ids.contiguous(), bias, out)
        return out
    h = w.numel()
    idx = torch.remainder(ids, h)
    z = w.reshape(-1)[idx].sum(1)
    if bias is not None:
        z = z + bias.reshape(())
    out.copy_(z.reshape(out.shape))
    return out


_M32 = 0xFFFFFFFF


def philox_u01(seed: int, ctr: torch.Tensor, ctr_hi: torch.Tensor | None = None) -> torch.Tensor:
    """uniform [0, 1) from the 4 words of Philox-4x32-10(seed, ctr) -> [n, 4] -- bit-identical
    to ``Philox::gen`` + ``u01`` in csrc/include/psamd_device.h (and the host copy in the native
    server), computed with int64 torch ops so the CPU oracle initialises rows exactly like the
    HIP kernel."""
    ctr = ctr.long()
    c0, c1 = ctr & _M32, (ctr >> 32) & _M32
    if ctr_hi is None:
        c2 = torch.zeros_like(c0)
        c3 = torch.zeros_like(c0)
    else:  # 128-bit counter: high 64 bits
        hi = ctr_hi.long().expand_as(ctr)
        c2, c3 = hi & _M32, (hi >> 32) & _M32
    k0, k1 = int(seed) & _M32, (int(seed) >> 32) & _M32
    for _ in range(10):
        p0 = 0xD2511F53 * c0  # < 2^64: wraps in int64 with the same low bits
        p1 = 0xCD9E8D57 * c2
        hi0, lo0 = (p0 >> 32) & _M32, p0 & _M32
        hi1, lo1 = (p1 >> 32) & _M32, p1 & _M32
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0 = (k0 + 0x9E3779B9) & _M32
        k1 = (k1 + 0xBB67AE85) & _M32
    return torch.stack([(c >> 8).float() * (1.0 / 16777216.0) for c in (c0, c1, c2, c3)], dim=-1)


def init_values(seed: int, keys: torch.Tensor, dim: int, lo: float, hi: float) -> torch.Tensor:
    """Deterministic first-touch values of rows ``keys`` ([n] int64 global keys) -> [n, dim]:
    element c is word c % 4 of Philox(seed, counter = (c // 4, key)) -- a 128-bit counter, so
    keys that differ only in their high (field) bits still get independent rows."""
    q = torch.arange((dim + 3) // 4, dtype=torch.int64, device=keys.device)
    ctr = q[None, :].expand(keys.numel(), -1)
    khi = keys.long()[:, None].expand_as(ctr)
    u = philox_u01(seed, ctr.reshape(-1), khi.reshape(-1)).reshape(keys.numel(), -1)[:, :dim]
    return lo + (hi - lo) * u


def lazy_init_rows(table: torch.Tensor, rows: torch.Tensor, flags: torch.Tensor, seed: int, row_base: int,
                   lo: float, hi: float, keys: torch.Tensor | None = None) -> None:
    """Initialise rows not yet touched (flags==0) deterministically from (seed, global key);
    the key is ``keys[r]`` when given, else ``rows[r] + row_base``.  Negative rows skipped."""
    if use_native(table, rows):
        native().lazy_init_rows(table, rows.contiguous(), flags, int(seed), int(row_base), float(lo), float(hi),
                                None if keys is None else keys.contiguous())
        return
    rows = rows.long()
    k = rows + row_base if keys is None else keys.long()
    ok = rows >= 0
    rows, k = rows[ok], k[ok]
    new = flags[rows] == 0
    rows, k = rows[new], k[new]
    if rows.numel():
        table[rows] = init_values(seed, k, table.shape[1], lo, hi).to(table.dtype)
        flags[rows] = 1


def hash_slots(hkeys: torch.Tensor, ids: torch.Tensor, insert: bool, status: torch.Tensor) -> torch.Tensor:
    """Slots of ``ids`` in the device open-addressing map ``hkeys`` (HIP kernel, GPU only)."""
    out = torch.empty_like(ids)
    native().hash_slots(hkeys, ids.contiguous(), out, bool(insert), status)
    return out


_M64 = (1 << 64) - 1


def _mix_key(x: int) -> int:
    """``mix_key`` of csrc/kernels/sparse.hip on a Python int (the map's probe start)."""
    x &= _M64
    x ^= x >> 33
    x = (x * 0xFF51AFD7ED558CCD) & _M64
    x ^= x >> 33
    x = (x * 0xC4CEB9FE1A85EC53) & _M64
    return x ^ (x >> 33)


def _probe_insert_cpu(new_hkeys: torch.Tensor, keys: torch.Tensor) -> torch.Tensor:
    """Host model of the device map's insertion (linear probing from ``mix_key``): slots of the
    unique ``keys`` in the CPU array ``new_hkeys``, -1 for pad keys (< 0)."""
    cap = new_hkeys.numel()
    hk = new_hkeys.tolist()
    pos = {k: i for i, k in enumerate(hk) if k >= 0}
    out = []
    for k in keys.tolist():
        if k < 0:
            out.append(-1)
            continue
        h = pos.get(k)
        if h is None:
            h = _mix_key(k) & (cap - 1)
            for _ in range(cap):
                if hk[h] < 0:
                    break
                h = (h + 1) & (cap - 1)
            else:
                h = -1
            if h >= 0:
                hk[h] = k
                pos[k] = h
        out.append(h)
    new_hkeys.copy_(torch.tensor(hk, dtype=torch.int64))
    return torch.tensor(out, dtype=torch.int64)


def rehash_rows_ref(old_hkeys, new_hkeys, old_table, new_table, old_flags, new_flags, old_states, new_states):
    """Oracle of ``rehash_rows`` as a composition: insert every old key into the new map
    (``hash_slots`` on the GPU -- the empty entries are pad keys -1 and resolve to slot -1 -- or
    the host model of the same probing on CPU tensors), then masked index copies."""
    if old_hkeys.is_cuda:
        status = torch.zeros(1, dtype=torch.int32, device=old_hkeys.device)
        remap = hash_slots(new_hkeys, old_hkeys, True, status)
    else:
        remap = _probe_insert_cpu(new_hkeys, old_hkeys)
    src = torch.nonzero(remap >= 0).reshape(-1)
    dst = remap[src]
    new_table[dst] = old_table[src]
    new_flags[dst] = old_flags[src]
    for o, n in zip(old_states, new_states):
        n[dst] = o[src]
    return remap


def rehash_rows(old_hkeys, new_hkeys, old_table, new_table, old_flags, new_flags, old_states=(), new_states=()):
    """Move a map-mode shard into a larger one in one pass (HIP on the GPU): every key of
    ``old_hkeys`` is inserted into ``new_hkeys`` (power-of-two capacity >= 2x, pre-filled with -1)
    and its table row, flag and state entries ([cap, dim] or row-wise [cap]) move to the new slot.
    The ``new_*`` tensors come zero-filled.  -> remap [old cap]: new slot of every old position,
    -1 where it was empty."""
    if new_hkeys.numel() < 2 * old_hkeys.numel():
        raise ValueError("rehash_rows: the new map must be at least twice the old one")
    if use_native(old_table, old_hkeys):
        remap = torch.empty_like(old_hkeys)
        native().rehash_rows(old_hkeys, new_hkeys, old_table, new_table, old_flags, new_flags, list(old_states),
                             list(new_states), remap)
        return remap
    return rehash_rows_ref(old_hkeys, new_hkeys, old_table, new_table, old_flags, new_flags, old_states, new_states)


def hash_slots_stamp(hkeys: torch.Tensor, ids: torch.Tensor, stamp: torch.Tensor, now: int, status: torch.Tensor, *,
                     cutoff: int | None = None, table: torch.Tensor | None = None,
                     flags: torch.Tensor | None = None, states=()) -> torch.Tensor:
    """``hash_slots`` with insert for tables whose rows expire (HIP kernel, GPU only): also
    ``stamp[slot] = now`` (int32 [capacity]) for every resolved slot; pad keys stamp nothing.
    With ``cutoff`` (and ``table`` / ``flags`` / ``states``) a key found with ``stamp < cutoff`` is
    reborn: row, flag and states of its slot are zeroed, the state of a slot never used."""
    out = torch.empty_like(ids)
    if cutoff is None:
        native().hash_slots_stamp(hkeys, ids.contiguous(), out, stamp, int(now), -(1 << 31), None, None, [], status)
    else:
        native().hash_slots_stamp(hkeys, ids.contiguous(), out, stamp, int(now), max(int(cutoff), -(1 << 31)), table,
                                  flags, list(states), status)
    return out


def _check_compact_cap(new_cap: int) -> None:
    if new_cap < 64 or new_cap & (new_cap - 1):
        raise ValueError(f"compact_rows: the new map needs a power-of-two capacity >= 64 (got {new_cap})")


def compact_rows_ref(old_hkeys, new_hkeys, old_table, new_table, old_flags, new_flags, old_stamp, new_stamp,
                     cutoff, counters, status, old_states=(), new_states=()):
    """Oracle of ``compact_rows`` as a composition: the keys of expired positions are masked to
    -1, the rest inserted into the new map (``hash_slots`` on the GPU, the host model of the same
    probing on CPU tensors), then masked index copies.  A survivor that finds the map full gets
    remap -1 and sets ``status``."""
    _check_compact_cap(new_hkeys.numel())
    live = old_hkeys >= 0
    keep = live & (old_stamp >= int(cutoff))
    masked = torch.where(keep, old_hkeys, torch.full_like(old_hkeys, -1))
    if old_hkeys.is_cuda:
        remap = hash_slots(new_hkeys, masked, True, status)
    else:
        remap = _probe_insert_cpu(new_hkeys, masked)
        if bool(((remap < 0) & keep).any()):
            status[0] = 1
    src = torch.nonzero(remap >= 0).reshape(-1)
    dst = remap[src]
    new_table[dst] = old_table[src]
    new_flags[dst] = old_flags[src]
    new_stamp[dst] = old_stamp[src]
    for o, n in zip(old_states, new_states):
        n[dst] = o[src]
    counters += torch.stack([(remap >= 0).sum(), (live & ~keep).sum()]).to(counters.dtype)
    return remap


def compact_rows(old_hkeys, new_hkeys, old_table, new_table, old_flags, new_flags, old_stamp, new_stamp, cutoff,
                 counters, status, old_states=(), new_states=()):
    """``rehash_rows`` with a filter (HIP on the GPU): an old position moves iff its key is live and
    ``old_stamp >= cutoff`` -- key, row, flag, states and stamp; the payload of an evicted position
    is not read.  ``new_hkeys`` (pre-filled with -1; the other ``new_*`` zero-filled) has any
    power-of-two capacity >= 64, smaller than the old one included; the caller sizes it so that the
    survivors fill at most half.  ``counters`` int64 [2] += (rows placed, rows evicted);
    ``status`` int32 [1] is set if a survivor found the map full.  -> remap [old cap]: the new slot,
    -1 for empty, evicted and unplaced positions."""
    _check_compact_cap(new_hkeys.numel())
    if use_native(old_table, old_hkeys):
        remap = torch.empty_like(old_hkeys)
        native().compact_rows(old_hkeys, new_hkeys, old_table, new_table, old_flags, new_flags, old_stamp, new_stamp,
                              int(cutoff), counters, status, list(old_states), list(new_states), remap)
        return remap
    return compact_rows_ref(old_hkeys, new_hkeys, old_table, new_table, old_flags, new_flags, old_stamp, new_stamp,
                            cutoff, counters, status, old_states, new_states)


class _GatherUnique(torch.autograd.Function):
    """out[k] = leaf[inv[k]] (cast to out_dtype); backward = deterministic segment sum of the
    output gradient per unique row (sorted-order perm + seg_off), no atomics, no sort."""

    @staticmethod
    def forward(ctx, leaf, inv, perm, seg_off, out_dtype):
        out = torch.empty(inv.numel(), leaf.shape[1], dtype=out_dtype, device=leaf.device)
        native().gather_rows(leaf, inv, out, 0, ACT_NONE)
        ctx.save_for_backward(perm, seg_off)
        ctx.nrows, ctx.ldtype = leaf.shape[0], leaf.dtype
        return out

    @staticmethod
    def backward(ctx, dout):
        perm, seg_off = ctx.saved_tensors
        dleaf = torch.empty(ctx.nrows, dout.shape[1], dtype=ctx.ldtype, device=dout.device)
        native().segment_reduce_rows(dout.contiguous(), perm, seg_off, dleaf, False)
        return dleaf, None, None, None, None


def unique_with_segments(ids: torch.Tensor):
    """(uniq, inv, counts, perm, seg_off) of a flat id vector: perm lists positions in sorted-id
    order (stable), seg_off[u]..seg_off[u+1] the occurrences of uniq[u] within perm."""
    ids = ids.reshape(-1)
    srt, perm = torch.sort(ids, stable=True)
    uniq, inv_sorted, counts = torch.unique_consecutive(srt, return_inverse=True, return_counts=True)
    inv = torch.empty_like(inv_sorted)
    inv[perm] = inv_sorted
    seg_off = torch.zeros(uniq.numel() + 1, dtype=torch.int64, device=ids.device)
    torch.cumsum(counts, 0, out=seg_off[1:])
    return uniq, inv, counts, perm, seg_off


def gather_unique(leaf: torch.Tensor, inv: torch.Tensor, perm: torch.Tensor, seg_off: torch.Tensor,
                  out_dtype=None) -> torch.Tensor:
    """leaf[inv] (optionally cast) with a segment-sum backward; GPU path = HIP gather_rows /
    segment_reduce_rows, CPU = torch indexing."""
    out_dtype = out_dtype or leaf.dtype
    if use_native(leaf, inv):
        return _GatherUnique.apply(leaf, inv.reshape(-1), perm, seg_off, out_dtype)
    return leaf[inv.reshape(-1)].to(out_dtype)


class _PoolUnique(torch.autograd.Function):
    """out[g] = s_g * sum_{j in bag g} weights[j] * leaf[inv[j]] (cast to out_dtype); backward = the
    deterministic per-unique-row sum of the scaled bag gradients (``bag_pool_bwd``).  Neither pass
    writes an [nnz, dim] tensor unless the ``bag_pool`` route is disabled."""

    @staticmethod
    def forward(ctx, leaf, inv, perm, seg_off, bag_off, bag_of, weights, mean, out_dtype):
        out = torch.empty(bag_off.numel() - 1, leaf.shape[1], dtype=out_dtype, device=leaf.device)
        bag_pool_fwd(leaf, inv, bag_off, out, weights, mean)
        ctx.save_for_backward(perm, seg_off, bag_off, bag_of, weights)
        ctx.nrows, ctx.mean = leaf.shape[0], bool(mean)
        return out

    @staticmethod
    def backward(ctx, dout):
        perm, seg_off, bag_off, bag_of, weights = ctx.saved_tensors
        dleaf = torch.empty(ctx.nrows, dout.shape[1], dtype=torch.float32, device=dout.device)
        bag_pool_bwd(dout.contiguous(), perm, seg_off, bag_of, bag_off, dleaf, weights, ctx.mean)
        return dleaf, None, None, None, None, None, None, None, None


def pool_unique(leaf: torch.Tensor, inv: torch.Tensor, perm: torch.Tensor, seg_off: torch.Tensor,
                bag_off: torch.Tensor, bag_of: torch.Tensor, weights: torch.Tensor | None = None,
                mean: bool = False, out_dtype=None) -> torch.Tensor:
    """Pooled ``gather_unique``: bag g (value positions bag_off[g] .. bag_off[g+1], ``bag_of`` their
    bag index) -> the sum (``mean``: the mean; ``weights``: the weighted sum) of leaf[inv[j]] over
    its values, [G, dim].  GPU path = the HIP bag kernels, CPU = differentiable torch ops.
    ``weights`` gets no gradient."""
    if weights is not None and weights.requires_grad:
        raise ValueError("pool_unique: weights get no gradient (detach them)")
    out_dtype = out_dtype or leaf.dtype
    inv = inv.reshape(-1)
    if use_native(leaf, inv):
        w = None if weights is None else weights.float().contiguous()
        return _PoolUnique.apply(leaf, inv, perm, seg_off, bag_off, bag_of, w, bool(mean), out_dtype)
    src = leaf[inv]
    if weights is not None:
        src = src * weights[:, None].to(src.dtype)
    out = torch.zeros(bag_off.numel() - 1, leaf.shape[1], dtype=leaf.dtype).index_add(0, bag_of, src)
    if mean:
        out = out * _bag_scale(bag_off)[:, None]
    return out.to(out_dtype)
