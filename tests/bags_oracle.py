"""fp64 oracles, error bounds and input builders for the multi-hot bag kernels
(``bag_pool_fwd`` / ``bag_pool_bwd``, csrc/kernels/bags.hip) and for ``lookup_bags``.

Bounds, in the form used for ``segment_reduce_rows``: a bag or segment of n terms t_j = w_j * x_j
is summed in fp32 in a fixed order; every term passes at most one rounding for the weight
multiply and n - 1 for the adds, so the result differs from the exact sum by at most
(n + 1) * 2^-24 * sum |t_j| (one unit of slack for the second-order terms).  Mean mode rounds
1 / len and multiplies by it: (n + 2).  A bf16 output adds its own rounding, 2^-8 * |ref|.  An
empty bag or segment has sum |t_j| = 0: the bound is 0, the result exactly zero."""
from dataclasses import dataclass
from typing import Optional

import torch

LENS = (0, 1, 2, 3, 4, 5, 9, 33)  # empty, every tail of the 4-way unroll, a long chain
EPS = 2.0 ** -24
BF16 = 2.0 ** -8


@dataclass
class BagCase:
    rows: torch.Tensor        # [nu, dim] fp32
    inv: torch.Tensor         # [nnz] unique-row index of every value
    bag_off: torch.Tensor     # [G + 1]
    bag_of: torch.Tensor      # [nnz] bag of every value
    perm: torch.Tensor        # [nnz] value positions sorted by unique row (stable)
    seg_off: torch.Tensor     # [nseg + 1]; segments past nu are the empty pads [nnz, nnz)
    weights: Optional[torch.Tensor]  # [nnz] fp32
    dout: torch.Tensor        # [G, dim] fp32

    @property
    def nbags(self):
        return self.bag_off.numel() - 1

    @property
    def nseg(self):
        return self.seg_off.numel() - 1


def check_indices(c: BagCase) -> None:
    """Every index a kernel will follow, checked on the CPU before anything runs on a GPU."""
    nnz, nu, G = c.inv.numel(), c.rows.shape[0], c.nbags
    for t in (c.inv, c.bag_off, c.bag_of, c.perm, c.seg_off):
        assert t.dtype == torch.int64 and t.dim() == 1
    assert c.bag_off[0] == 0 and c.bag_off[-1] == nnz and bool((c.bag_off[1:] >= c.bag_off[:-1]).all())
    assert c.seg_off[0] == 0 and c.seg_off[-1] == nnz and bool((c.seg_off[1:] >= c.seg_off[:-1]).all())
    assert c.bag_of.numel() == nnz and c.perm.numel() == nnz
    if nnz:
        assert 0 <= int(c.inv.min()) and int(c.inv.max()) < nu
        assert 0 <= int(c.bag_of.min()) and int(c.bag_of.max()) < G
        assert torch.equal(torch.sort(c.perm).values, torch.arange(nnz))
        pos = torch.arange(nnz)
        assert bool((c.bag_off[c.bag_of] <= pos).all()) and bool((pos < c.bag_off[c.bag_of + 1]).all())
        seg_of = torch.repeat_interleave(torch.arange(c.nseg), c.seg_off[1:] - c.seg_off[:-1])
        assert torch.equal(c.inv[c.perm], seg_of)  # segment u lists exactly the values of row u
    assert c.nseg >= nu and c.dout.shape == (G, c.rows.shape[1])
    if c.weights is not None:
        assert c.weights.shape == (nnz,) and c.weights.dtype == torch.float32


def make_case(dim: int, nbags: int = 300, nu: int = 97, seed: int = 0, weights: bool = False,
              pad_segments: bool = True, lens=LENS, hot_bags: int = 70) -> BagCase:
    """Bags with lengths drawn from ``lens``; a leading and a trailing empty bag; one id repeated
    inside one bag; hot row 0 in ``hot_bags`` (> 64) different bags -> a long backward segment;
    rows that no value uses -> empty segments; with ``pad_segments`` the segment list is padded to
    nnz entries by empty segments [nnz, nnz), like the sync-free W = 1 plan."""
    g = torch.Generator().manual_seed(seed)
    choice = torch.tensor(lens)
    ln = choice[torch.randint(0, len(lens), (nbags,), generator=g)]
    ln[1:1 + len(lens)] = choice  # every length occurs
    ln[0] = 0
    ln[-1] = 0
    bag_off = torch.zeros(nbags + 1, dtype=torch.int64)
    torch.cumsum(ln, 0, out=bag_off[1:])
    nnz = int(bag_off[-1])
    inv = torch.randint(1, nu - 3, (nnz,), generator=g)  # rows nu-3 .. nu-1 stay unused
    nonempty = torch.nonzero(ln > 0).reshape(-1)
    assert nonempty.numel() >= hot_bags > 64
    inv[bag_off[nonempty[:hot_bags]]] = 0  # row 0: first value of hot_bags bags
    rep = int(torch.nonzero(ln >= 3).reshape(-1)[0])
    inv[bag_off[rep] + 2] = inv[bag_off[rep] + 1]  # the same id twice in one bag
    bag_of = torch.repeat_interleave(torch.arange(nbags), ln)
    perm = torch.argsort(inv, stable=True)
    cnt = torch.bincount(inv, minlength=nu)
    seg_off = torch.zeros(nu + 1, dtype=torch.int64)
    torch.cumsum(cnt, 0, out=seg_off[1:])
    if pad_segments and nnz > nu:
        seg_off = torch.cat([seg_off, torch.full((nnz - nu,), nnz, dtype=torch.int64)])
    c = BagCase(rows=torch.randn(nu, dim, generator=g), inv=inv, bag_off=bag_off, bag_of=bag_of, perm=perm,
                seg_off=seg_off, weights=(torch.rand(nnz, generator=g) * 2 - 0.5) if weights else None,
                dout=torch.randn(nbags, dim, generator=g))
    check_indices(c)
    assert int(cnt[0]) > 64 and int(cnt[nu - 1]) == 0
    return c


def _scale64(bag_off: torch.Tensor, mean: bool) -> torch.Tensor:
    ln = (bag_off[1:] - bag_off[:-1]).clamp(min=1).double()
    return 1.0 / ln if mean else torch.ones_like(ln)


def oracle_fwd(rows, inv, bag_off, bag_of, weights=None, mean=False):
    """-> (ref [G, dim] fp64, mag = s_g * sum |w x| [G, dim] fp64, n terms per bag [G])."""
    G = bag_off.numel() - 1
    t = rows.double()[inv]
    if weights is not None:
        t = t * weights.double()[:, None]
    s = _scale64(bag_off, mean)[:, None]
    ref = torch.zeros(G, rows.shape[1], dtype=torch.float64).index_add_(0, bag_of, t) * s
    mag = torch.zeros(G, rows.shape[1], dtype=torch.float64).index_add_(0, bag_of, t.abs()) * s
    return ref, mag, bag_off[1:] - bag_off[:-1]


def oracle_bwd(dout, perm, seg_off, bag_of, bag_off, weights=None, mean=False):
    """-> (ref [nseg, dim] fp64, mag [nseg, dim] fp64, n terms per segment [nseg]); ``dout`` may be
    bf16 (its values are exact in fp64)."""
    nseg = seg_off.numel() - 1
    sc = _scale64(bag_off, mean)[bag_of]
    if weights is not None:
        sc = sc * weights.double()
    t = (dout.double()[bag_of] * sc[:, None])[perm]
    n = seg_off[1:] - seg_off[:-1]
    seg_of = torch.repeat_interleave(torch.arange(nseg), n)
    ref = torch.zeros(nseg, dout.shape[1], dtype=torch.float64).index_add_(0, seg_of, t)
    mag = torch.zeros(nseg, dout.shape[1], dtype=torch.float64).index_add_(0, seg_of, t.abs())
    return ref, mag, n


def bound(ref, mag, n, mean: bool, bf16_out: bool = False) -> torch.Tensor:
    b = (n.double() + (2 if mean else 1))[:, None] * EPS * mag
    if bf16_out:
        b = b + BF16 * ref.abs()
    return b


def assert_within(got: torch.Tensor, ref, mag, n, mean: bool, what: str = "") -> None:
    """Per element: |got - ref| <= bound; rows of empty bags / segments exactly zero."""
    got = got.detach().cpu()
    b = bound(ref, mag, n, mean, got.dtype == torch.bfloat16)
    err = (got.double() - ref).abs()
    worst = float((err - b).max()) if err.numel() else 0.0
    assert bool((err <= b).all()), f"{what}: worst excess over the bound {worst:.3e} (max err {float(err.max()):.3e})"
    empty = n == 0
    if bool(empty.any()):
        assert bool((got[empty] == 0).all()), f"{what}: an empty bag / segment is not exactly zero"


def make_bags(samples: int, fields: int, id_hi: int, seed: int = 0, lens=LENS, weights: bool = False):
    """Multi-hot input of a table: (values [nnz], offsets [samples*fields + 1][, weights]); ids in
    [0, id_hi) skewed to small ids, first and last bag empty."""
    g = torch.Generator().manual_seed(seed)
    G = samples * fields
    ln = torch.tensor(lens)[torch.randint(0, len(lens), (G,), generator=g)]
    ln[0] = 0
    ln[-1] = 0
    offsets = torch.zeros(G + 1, dtype=torch.int64)
    torch.cumsum(ln, 0, out=offsets[1:])
    nnz = int(offsets[-1])
    values = (torch.rand(nnz, generator=g).pow(2) * id_hi).long().clamp_(0, id_hi - 1)
    assert offsets[0] == 0 and offsets[-1] == values.numel() and bool((values >= 0).all()) and bool((values < id_hi).all())
    if weights:
        return values, offsets, torch.rand(nnz, generator=g) + 0.5
    return values, offsets


def slice_bags(values, offsets, fields: int, lo: int, hi: int, weights=None):
    """The bags of samples lo .. hi-1 as an input of their own."""
    a, b = int(offsets[lo * fields]), int(offsets[hi * fields])
    off = offsets[lo * fields:hi * fields + 1] - a
    if weights is not None:
        return values[a:b].clone(), off.clone(), weights[a:b].clone()
    return values[a:b].clone(), off.clone()
