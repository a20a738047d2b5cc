"""fp64 oracles and input builders for the sparse-row kernels (csrc/kernels/sparse.hip from
gather_rows_kernel to row_plane_accum_kernel, and sparse_opt_kernel / sparse_opt_vec_kernel in
csrc/kernels/optim.hip).  Plain torch on the CPU; imported by test_rows_oracle_cpu.py and
test_rows_gpu.py.

The oracles are written from the kernels' comments and opt_apply<KIND>, not from the project's
fp32 CPU paths (ops/optim.py::_apply_ref, the CPU branches of ops/sparse.py), and are vectorised:
index_add_ in fp64, no Python loop per row.

Every builder asserts, before anything can be launched, that each non-negative index it returns is
inside the array it indexes: the kernels do not bounds-check.

Which kernel a row width reaches (lg = log2(dim / 4) when dim = 4 * 2^lg <= 256):

    dim   sparse_opt             segment_reduce_rows   gather_rows (fp32 table, aligned slice)   lazy_init_rows
    4     vec, lg 0, 64 rows/wave   vec, lg 0          lg kernel (fp32 / bf16 out)              L = 1, P = 64
    16    vec, lg 2                 vec, lg 2          lg kernel                                L = 4, P = 16
    128   vec, lg 5 (DLRM)          vec, lg 5          lg kernel                                L = 32, P = 2
    256   vec, lg 6, 1 row/wave     vec, lg 6          lg kernel                                L = 64, P = 1
    12    scalar (3 lanes)          scalar             vec4 (fp32 out), generic (bf16 out)      one row per wave
    10    scalar (CTR)              scalar             generic                                  one row per wave
    260   scalar (> 256)            scalar             vec4 (fp32 out), generic (bf16 out)      one row per wave

A bf16 table, or a column slice whose offset is not a multiple of 4, sends gather_rows to the
generic kernel at every width; a table, state or gradient base that is not 16-byte aligned sends
sparse_opt to the scalar kernel at every width.
"""
import torch

SGD, ADAM, ADAGRAD, FTRL = 0, 1, 2, 3
ACT_NONE, ACT_RELU, ACT_LEAKY, ACT_SIGMOID = 0, 1, 2, 3

U24 = 2.0 ** -24  # half an fp32 ulp, relative: one fp32 rounding
U8 = 2.0 ** -8    # one bf16 rounding is within 2^-9 relative; 2^-8 leaves room for the fp32 error under it

_HP_DEFAULT = dict(lr=0.01, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.0, momentum=0.0, dampening=0.0, nesterov=False,
                   adamw=False, bc1=1.0, bc2=1.0, l1=0.0, l2=0.0, fbeta=1.0, ftrl_mode=0, gscale=1.0)

_T = 3  # the step the Adam sets stand at: bc = 1 / (1 - beta^t)
_BC = dict(bc1=1.0 / (1.0 - 0.9 ** _T), bc2=1.0 / (1.0 - 0.999 ** _T))
_BASE = dict(lr=0.05, eps=1e-6, gscale=0.5)

# name -> (kind, rowwise, skip_zero, hyper-parameters): every branch of opt_apply<KIND>
HP_SETS = {
    "sgd": (SGD, False, False, dict(_BASE)),
    "sgd_momentum": (SGD, False, False, dict(_BASE, wd=0.01, momentum=0.9, dampening=0.1)),
    "sgd_nesterov": (SGD, False, False, dict(_BASE, wd=0.01, momentum=0.9, nesterov=True)),
    "adam": (ADAM, False, False, dict(_BASE, wd=0.01, **_BC)),
    "adamw": (ADAM, False, False, dict(_BASE, wd=0.1, adamw=True, **_BC)),
    "adagrad": (ADAGRAD, False, False, dict(_BASE, wd=0.01)),
    "adagrad_rowwise": (ADAGRAD, True, False, dict(_BASE)),
    "ftrl0": (FTRL, False, False, dict(_BASE, l1=0.01, l2=0.01, fbeta=1.0, ftrl_mode=0)),
    "ftrl1_skip": (FTRL, False, True, dict(_BASE, l1=0.01, l2=0.01, fbeta=1.0, ftrl_mode=1)),
}
SPARSE_HP = tuple(HP_SETS)  # the sets the sparse-row cases run (and seed by): fixed, whatever is added below
# the dense shard tests (dense_oracle.py) add FTRL at l1 = 0.5, where randn z puts a large share of the
# elements on either side of the |z| <= l1 branch; the other dense sets are the sparse ones
HP_SETS.update({
    "ftrl0_dense": (FTRL, False, False, dict(_BASE, l1=0.5, l2=0.01, fbeta=1.0, ftrl_mode=0)),
    "ftrl1_dense": (FTRL, False, False, dict(_BASE, l1=0.5, l2=0.01, fbeta=1.0, ftrl_mode=1)),
})
DENSE_HP = ("sgd", "sgd_momentum", "sgd_nesterov", "adam", "adamw", "adagrad", "ftrl0_dense", "ftrl1_dense")
HP_SHORT = ("adagrad_rowwise", "adam", "ftrl1_skip")
OPT_DIMS = (4, 16, 128, 256, 12, 10, 260)
OPT_DIMS_ALL_HP = (10, 128)
FORMS = ("unique", "runs", "plane")
GDTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}


def opt_cases():
    """(dim, gradient dtype, hyper-parameter set, form) of every small sparse_opt case."""
    out = []
    for dim in OPT_DIMS:
        for hp in (SPARSE_HP if dim in OPT_DIMS_ALL_HP else HP_SHORT):
            for gdt in GDTYPES:
                for form in FORMS:
                    out.append((dim, gdt, hp, form))
    return out


# ------------------------------------------------------------------------------------ builders
def check_rows(idx, bound):
    """Every index is -1 (a pad) or inside [0, bound)."""
    idx = torch.as_tensor(idx)
    assert idx.dtype == torch.int64
    assert bool(((idx >= -1) & (idx < bound)).all()), f"index outside [-1, {bound})"
    return idx


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def build_unique_rows(n, rows_total, seed, live=None):
    """n entries: `live` distinct rows at random positions, -1 pads everywhere else."""
    g = _gen(seed)
    live = min(n, rows_total * 5 // 6) if live is None else live
    assert live <= min(n, rows_total)
    rows = torch.full((n,), -1, dtype=torch.int64)
    rows[torch.randperm(n, generator=g)[:live]] = torch.randperm(rows_total, generator=g)[:live]
    return check_rows(rows, rows_total)


_RUN_LENS = (1, 2, 3, 4, 5, 5, 4)  # mean 3.4: 900 entries stay under 300 distinct rows


def build_sorted_runs(n, rows_total, seed, pads=20, long_run=40):
    """n sorted entries: `pads` -1s, runs of 1-5, and one run of `long_run` that starts 14 entries
    before a 64-entry boundary (so its head's walk leaves the wave step it began in)."""
    g = _gen(seed)
    lens, total, long_at = [], pads, None
    while total < n:
        if long_at is None and total >= 50 and (total % 64) >= 50 and total + long_run <= n:
            long_at = len(lens)
            lens.append(long_run)
        else:
            lens.append(min(_RUN_LENS[int(torch.randint(0, len(_RUN_LENS), (1,), generator=g))], n - total))
        total += lens[-1]
    assert long_at is not None and len(lens) <= rows_total - 8, (len(lens), rows_total)
    ids = torch.sort(torch.randperm(rows_total, generator=g)[:len(lens)]).values
    rows = torch.cat([torch.full((pads,), -1, dtype=torch.int64), torch.repeat_interleave(ids, torch.tensor(lens))])
    assert rows.numel() == n
    start = pads + sum(lens[:long_at])
    assert start // 64 != (start + long_run - 1) // 64  # the long run straddles a 64-entry boundary
    return check_rows(rows, rows_total)


def build_random_runs(n, rows_total, seed):
    """n sorted entries drawn with repeats (a few -1): the large grid-wrap inputs."""
    rows = torch.randint(0, rows_total, (n,), generator=_gen(seed))
    rows[::97] = -1
    return check_rows(torch.sort(rows).values, rows_total)


def build_touched(n, rows_total, seed, ncount):
    """The row-plane form: entries [0, ncount) are distinct rows in arbitrary order; what follows is
    stale but valid-looking (first the last live row again, then rows of which some are named
    nowhere else, then -1) and must not be read."""
    g = _gen(seed)
    assert ncount <= rows_total - 20 and ncount < n
    p = torch.randperm(rows_total, generator=g)
    t = torch.full((n,), -1, dtype=torch.int64)
    t[:ncount] = p[:ncount]
    t[ncount] = p[ncount - 1]
    stale = p[ncount - 10:ncount + 10]
    t[ncount + 1:ncount + 1 + stale.numel()] = stale
    return check_rows(t, min(rows_total, n))  # touched indexes the table AND the gradient rows


def build_grad(n, dim, dtype, seed, zero_every=11):
    """randn rows with an exact zero in column 0 on every `zero_every`-th entry."""
    g = torch.randn(n, dim, generator=_gen(seed))
    g[::zero_every, 0] = 0.0
    return g.to(dtype)


def build_states(kind, rowwise, rows_total, dim, seed, momentum=0.0):
    """(st0, st1) as the kind needs them; second moments / accumulators are rand + 0.1."""
    g = _gen(seed)
    pos = lambda *s: torch.rand(*s, generator=g) + 0.1  # noqa: E731
    if kind == SGD:
        return (torch.randn(rows_total, dim, generator=g) if momentum else None), None
    if kind == ADAM:
        return 0.1 * torch.randn(rows_total, dim, generator=g), pos(rows_total, dim)
    if kind == ADAGRAD:
        return (pos(rows_total) if rowwise else pos(rows_total, dim)), None
    return torch.randn(rows_total, dim, generator=g), pos(rows_total, dim)  # FTRL: z, n


def build_opt(dim, gdt, hpname, form, rows_total=300, n=900, seed=0):
    """One sparse_opt case: dict(kind, rowwise, skip_zero, hp, table, st0, st1, rows, grad, perm,
    ncount (int or None), named (bool [rows_total]: rows the live entries name))."""
    kind, rowwise, skip_zero, hp = HP_SETS[hpname]
    seed = seed + 1000 * dim + 7 * sorted(SPARSE_HP).index(hpname)
    table = torch.randn(rows_total, dim, generator=_gen(seed + 1))
    st0, st1 = build_states(kind, rowwise, rows_total, dim, seed + 2, hp.get("momentum", 0.0))
    grad = build_grad(n, dim, GDTYPES[gdt], seed + 3)
    perm, ncount = None, None
    if form == "unique":
        rows = build_unique_rows(n, rows_total, seed + 4)
    elif form == "runs":
        rows = build_sorted_runs(n, rows_total, seed + 4)
        perm = check_rows(torch.randperm(n, generator=_gen(seed + 5)), n)
        head = torch.ones(n, dtype=torch.bool)
        head[1:] = rows[1:] != rows[:-1]
        z = grad.clone()  # whole runs with a zero first element, so skip_zero meets runs longer than 1
        z[perm[torch.isin(rows, rows[head][3::7])], 0] = 0
        grad = z
    elif form == "plane":
        ncount = 211
        rows = build_touched(n, rows_total, seed + 4, ncount)
        perm = rows
    else:
        raise ValueError(form)
    live = rows if ncount is None else rows[:ncount]
    named = torch.zeros(rows_total, dtype=torch.bool)
    named[live[live >= 0]] = True
    assert int((~named).sum()) >= 8
    return dict(kind=kind, rowwise=rowwise, skip_zero=skip_zero, hp=dict(hp), table=table, st0=st0, st1=st1,
                rows=rows, grad=grad, perm=perm, ncount=ncount, named=named)


def build_opt_wrap(dim, n, rows_total=6000, seed=77):
    """Sorted runs with repeats, large enough to leave the 2048-block grid: Adagrad row-wise at the
    vectorised widths, Adam elsewhere."""
    hpname = "adagrad_rowwise" if dim == 128 else "adam"
    kind, rowwise, skip_zero, hp = HP_SETS[hpname]
    table = torch.randn(rows_total, dim, generator=_gen(seed + 1))
    st0, st1 = build_states(kind, rowwise, rows_total, dim, seed + 2)
    rows = build_random_runs(n, rows_total, seed + 3)
    perm = check_rows(torch.randperm(n, generator=_gen(seed + 4)), n)
    named = torch.zeros(rows_total, dtype=torch.bool)
    named[rows[rows >= 0]] = True
    return dict(kind=kind, rowwise=rowwise, skip_zero=skip_zero, hp=dict(hp), table=table, st0=st0, st1=st1,
                rows=rows, grad=build_grad(n, dim, torch.float32, seed + 5), perm=perm, ncount=None, named=named)


SEG_LENS = (0, 1, 3, 4, 5, 8, 41)


def build_segments(nseg, nsrc_rows, seed, lens=SEG_LENS):
    """(perm, seg_off): segment u has length lens[u % len(lens)]; perm lists each source row once
    (what torch.argsort gives dedup_rows), so nsrc_rows is the sum of the lengths."""
    ln = torch.tensor([lens[u % len(lens)] for u in range(nseg)], dtype=torch.int64)
    assert int(ln.sum()) == nsrc_rows
    seg_off = torch.zeros(nseg + 1, dtype=torch.int64)
    seg_off[1:] = torch.cumsum(ln, 0)
    perm = check_rows(torch.randperm(nsrc_rows, generator=_gen(seed)), nsrc_rows)
    assert bool((seg_off[1:] >= seg_off[:-1]).all()) and int(seg_off[-1]) == perm.numel()
    return perm, seg_off


def seg_rows(nseg, lens=SEG_LENS):
    return sum(lens[u % len(lens)] for u in range(nseg))


# ------------------------------------------------------------------------------------- oracles
def _apply64(kind, w, a, b, g, h):
    """opt_apply<KIND> element-wise in fp64; returns (w, st0, st1)."""
    lr = h["lr"]
    if kind == SGD:
        if h["wd"] != 0:
            g = g + h["wd"] * w
        if h["momentum"] != 0:
            a = h["momentum"] * a + (1.0 - h["dampening"]) * g
            g = g + h["momentum"] * a if h["nesterov"] else a
        return w - lr * g, a, b
    if kind == ADAM:
        if h["wd"] != 0 and not h["adamw"]:
            g = g + h["wd"] * w
        a = h["beta1"] * a + (1.0 - h["beta1"]) * g
        b = h["beta2"] * b + (1.0 - h["beta2"]) * g * g
        upd = (a * h["bc1"]) / (torch.sqrt(b * h["bc2"]) + h["eps"])  # eps outside the sqrt of v_hat
        if h["wd"] != 0 and h["adamw"]:
            upd = upd + h["wd"] * w
        return w - lr * upd, a, b
    if kind == ADAGRAD:
        if h["wd"] != 0:
            g = g + h["wd"] * w
        a = a + g * g
        return w - lr * g / (torch.sqrt(a) + h["eps"]), a, b
    if kind == FTRL:
        z, n, l1, l2, fb = a, b, h["l1"], h["l2"], h["fbeta"]
        if h["ftrl_mode"] == 1:  # w from (z, n_old); then sigma = sqrt(n + g^2) - sqrt(n / alpha)
            sgn = torch.where(z >= 0, 1.0, -1.0).double()
            wn = torch.where(z.abs() <= l1, torch.zeros_like(z), -(z - sgn * l1) / ((l2 + (fb + torch.sqrt(n))) / lr))
            sigma = torch.sqrt(n + g * g) - torch.sqrt(n / lr)
            return wn, z + (g - sigma * wn), n + g * g
        nn = n + g * g
        zn = z + g - (torch.sqrt(nn) - torch.sqrt(n)) / lr * w
        sgn = torch.where(zn >= 0, 1.0, -1.0).double()
        wn = torch.where(zn.abs() <= l1, torch.zeros_like(zn), -(zn - sgn * l1) / ((fb + torch.sqrt(nn)) / lr + l2))
        return wn, zn, nn
    raise ValueError(kind)


def sparse_opt64(kind, table, st0, st1, rows, grad, perm=None, rowwise=False, skip_zero=False, ncount=None, **hp):
    """(table, st0, st1) in fp64 after one row-sparse step; inputs are left unchanged.  Only
    rows[:ncount] are live.  perm None: grad row r belongs to rows[r].  perm given: grad row perm[j]
    belongs to rows[j], every run of equal adjacent rows is summed (fp64, over the fp32 / bf16
    values as given) and applied once.  Negative rows are skipped; skip_zero skips a row whose
    scaled run sum has an exact zero first element.  Row-wise Adagrad keeps one accumulator per row
    (mean of g^2 over the row) and takes neither weight decay nor skip_zero, as in the kernels."""
    h = dict(_HP_DEFAULT)
    assert not set(hp) - set(h), sorted(set(hp) - set(h))
    h.update(hp)
    T = table.double().clone()
    A = st0.double().clone() if st0 is not None else None
    B = st1.double().clone() if st1 is not None else None
    dim = T.shape[1]
    n = rows.numel() if ncount is None else min(int(ncount), rows.numel())
    rows = rows[:n]
    g = grad.double().reshape(-1, dim)
    if perm is None:
        g = g[:n]
    elif n:
        g = g[perm[:n]]
        head = torch.ones(n, dtype=torch.bool)
        head[1:] = rows[1:] != rows[:-1]
        seg = torch.cumsum(head.long(), 0) - 1
        g = torch.zeros(int(seg[-1]) + 1, dim, dtype=torch.float64).index_add_(0, seg, g)
        rows = rows[head]
    g = g * h["gscale"]
    keep = rows >= 0
    if kind == ADAGRAD and rowwise:
        rows, g = rows[keep], g[keep]
        assert rows.unique().numel() == rows.numel()
        A[rows] = A[rows] + (g * g).mean(dim=1)
        T[rows] = T[rows] - h["lr"] * g / (torch.sqrt(A[rows]) + h["eps"])[:, None]
        return T, A, B
    if skip_zero:
        keep = keep & (g[:, 0] != 0)
    rows, g = rows[keep], g[keep]
    assert rows.unique().numel() == rows.numel()
    zero = torch.zeros_like(g)
    w, a, b = _apply64(kind, T[rows], A[rows] if A is not None else zero, B[rows] if B is not None else zero, g, h)
    T[rows] = w
    if A is not None:
        A[rows] = a
    if B is not None:
        B[rows] = b
    return T, A, B


def segment_reduce64(src, perm, seg_off, mean=False):
    """(out, sumabs, count) in fp64: out[u] = sum (or mean; an empty segment divides by 1) of
    src[perm[j]] over j in [seg_off[u], seg_off[u + 1]); sumabs the same sum over |src| (undivided);
    count the segment lengths."""
    cnt = seg_off[1:] - seg_off[:-1]
    seg = torch.repeat_interleave(torch.arange(cnt.numel()), cnt)
    x = src.double()[perm[:int(seg_off[-1])]] if perm.numel() else src.double()[:0]
    out = torch.zeros(cnt.numel(), src.shape[1], dtype=torch.float64).index_add_(0, seg, x)
    sumabs = torch.zeros_like(out).index_add_(0, seg, x.abs())
    if mean:
        out = out / cnt.clamp(min=1).double()[:, None]
    return out, sumabs, cnt


def segment_bound(ref, sumabs, cnt, mean, out_bf16):
    """|out - ref| allowed per element: a segment of n rows takes at most n - 1 fp32 additions, and
    the mean two more roundings (the reciprocal, the product): (n + 1) 2^-24 sum|x|, scaled like
    the output; a bf16 output adds 2^-8 |ref|."""
    b = (cnt.double() + 1.0)[:, None] * U24 * sumabs
    if mean:
        b = b / cnt.clamp(min=1).double()[:, None]
    return b + (U8 * ref.abs() if out_bf16 else 0.0)


def act64(x, act):
    """apply_act in fp64."""
    if act == ACT_RELU:
        return torch.where(x > 0, x, torch.zeros_like(x))
    if act == ACT_LEAKY:
        return torch.where(x > 0, x, 0.01 * x)
    if act == ACT_SIGMOID:
        return 0.001 + 0.998 / (1.0 + torch.exp(-x))
    return x


def gather64(table, rows, act=ACT_NONE):
    """act(table[rows]) in fp64; a negative row gives a zero row (not act(0))."""
    ok = rows >= 0
    out = torch.zeros(rows.numel(), table.shape[1], dtype=torch.float64)
    out[ok] = act64(table.double()[rows[ok]], act)
    return out


def bf16_ulp(ref):
    """The spacing of bf16 numbers at |ref| (fp64 tensor)."""
    _, e = torch.frexp(ref.abs().clamp(min=2.0 ** -120))
    return torch.ldexp(torch.ones_like(ref), e - 8)


# ------------------------------------------------------------------------------------ row plane
def row_plane_recv_ref(skeys, meta, me, cap):
    """(rkeys [W * cap], pmeta [2 W]) of owner `me`: entry e is worker e // cap's key e % cap for this
    owner, read at that worker's offset meta[w][me], and -1 past its count meta[w][W + me]; pmeta
    holds the W (offset, count) pairs."""
    W = len(skeys)
    rkeys = torch.full((W * cap,), -1, dtype=torch.int64)
    pmeta = torch.zeros(2 * W, dtype=torch.int64)
    for w in range(W):
        off, cnt = int(meta[w][me]), int(meta[w][W + me])
        rkeys[w * cap:w * cap + cnt] = skeys[w][off:off + cnt]
        pmeta[2 * w], pmeta[2 * w + 1] = off, cnt
    return rkeys, pmeta


def row_plane_send_ref(table, rslots, pmeta, arenas, cap):
    """The workers' row arenas after the send: arena w row off + j = table[rslots[w * cap + j]] for
    j < cnt (a zero row for a slot < 0); every other arena row as it was."""
    out = [a.clone() for a in arenas]
    for w in range(len(arenas)):
        off, cnt = int(pmeta[2 * w]), int(pmeta[2 * w + 1])
        s = rslots[w * cap:w * cap + cnt]
        rows = torch.zeros(cnt, table.shape[1], dtype=table.dtype)
        rows[s >= 0] = table[s[s >= 0]]
        out[w][off:off + cnt] = rows
    return out


def row_plane_accum_ref(grads, rslots, pmeta, acc, tflag, tag, cap):
    """(acc fp64, tflag, touched set) after one accumulate pass over the W workers in rank order: a
    slot whose flag is not `tag` is overwritten and joins the touched set, a slot seen before in
    this round is added to.  A worker names a slot at most once."""
    acc, tflag, touched = acc.double().clone(), tflag.clone(), set()
    for w in range(len(grads)):
        off, cnt = int(pmeta[2 * w]), int(pmeta[2 * w + 1])
        s = rslots[w * cap:w * cap + cnt]
        ok = s >= 0
        s, g = s[ok], grads[w].double()[off:off + cnt][ok]
        assert s.unique().numel() == s.numel()
        first = tflag[s] != tag
        acc[s[first]] = g[first]
        acc[s[~first]] += g[~first]
        tflag[s] = tag
        touched.update(s[first].tolist())
    return acc, tflag, touched


def build_plane(dim, counts, cap, table_rows, seed, me=1):
    """W = len(counts) workers' arenas as one process sees them.  Worker w keeps its keys for owner
    `me` at offset offs[w] of its key arena, and its rows / gradients at the same offset of those
    arenas.  Keys are slots of a [table_rows, dim] table.  Worker 1's keys are drawn so that some
    are shared with one other worker and, when all three have keys, some with both."""
    g = _gen(seed)
    W = len(counts)
    offs = [5 + 3 * w for w in range(W)]
    pool = torch.randperm(table_rows, generator=g)
    pool = pool[(pool % 7 != 3) & (pool % 5 != 3)]  # keys that plane_slots(., 7) and (., 5) resolve
    common = pool[:max(1, min(c for c in counts if c) // 3)]  # keys every worker with keys begins with
    skeys, meta, grads, grads2, arenas = [], [], [], [], []
    for w, cnt in enumerate(counts):
        assert cnt <= cap and cnt <= table_rows
        own = torch.randperm(table_rows, generator=g)
        own = own[~torch.isin(own, common)]
        keys = torch.cat([common, own])[:cnt]
        keys = keys[torch.randperm(cnt, generator=g)]
        assert keys.unique().numel() == cnt
        arena = torch.full((offs[w] + cnt + 9,), -7, dtype=torch.int64)  # -7: never a key that is read
        arena[offs[w]:offs[w] + cnt] = keys
        skeys.append(arena)
        m = torch.full((2 * W,), 0, dtype=torch.int64)
        m[me], m[W + me] = offs[w], cnt
        # the other owners' segments of this worker: offsets / counts the kernel must not use
        for o in range(W):
            if o != me:
                m[o], m[W + o] = 1, 2
        meta.append(m)
        n = offs[w] + cnt + 9
        grads.append(torch.randn(n, dim, generator=g))
        grads2.append(torch.randn(n, dim, generator=g))
        arenas.append(torch.full((n, dim), -3.0))
        check_rows(keys, table_rows)
        assert offs[w] + cnt <= n
    table = torch.randn(table_rows, dim, generator=g)
    return dict(W=W, me=me, cap=cap, dim=dim, counts=list(counts), offs=offs, skeys=skeys, meta=meta, grads=grads,
                grads2=grads2, arenas=arenas, table=table)


def plane_slots(rkeys, m):
    """Owner-side slots of received keys: the key itself; keys with key % m == 3 stay unresolved (for
    every worker that sent them)."""
    s = rkeys.clone()
    s[(s >= 0) & (s % m == 3)] = -1
    return s


# (dim, per-worker counts, cap, table rows).  cap 512 is one accumulate block per worker; the last case
# has two (kAccChunk = 1024 entries each), so the touched list is reserved by more than one block.
PLANE_CASES = [(dim, counts, 512, 1024) for dim in (128, 12, 10, 260) for counts in ((0, 37, 512), (300, 1, 255))]
PLANE_CASES.append((128, (1500, 2048, 700), 2048, 4096))


def build_plane_case(dim, counts, cap, table_rows):
    return build_plane(dim, counts, cap, table_rows, 40 + dim)


def plane_apply_set(dim):
    """The optimizer the row-plane tests apply to the accumulator: DLRM's at DLRM's width."""
    return "adagrad_rowwise" if dim == 128 else ("ftrl0" if dim == 10 else "adam")


def plane_rounds_ref(p):
    """The exchange of test_row_plane by the references alone: (rslots, rslots2, acc fp32 after the
    second round, its touched list padded with -1 to the table's rows, the live count)."""
    rows = p["table"].shape[0]
    rkeys, pmeta = row_plane_recv_ref(p["skeys"], p["meta"], p["me"], p["cap"])
    rslots = check_rows(plane_slots(rkeys, 7), rows)
    rslots2 = check_rows(plane_slots(rslots, 5), rows)
    acc = torch.full((rows, p["dim"]), 100.0)
    flags = torch.zeros(rows, dtype=torch.int32)
    acc, flags, _ = row_plane_accum_ref(p["grads"], rslots, pmeta, acc, flags, 1, p["cap"])
    acc, flags, tset = row_plane_accum_ref(p["grads2"], rslots2, pmeta, acc.float(), flags, 2, p["cap"])
    touched = torch.full((rows,), -1, dtype=torch.int64)
    touched[:len(tset)] = torch.tensor(sorted(tset), dtype=torch.int64).flip(0)
    return rslots, rslots2, acc.float(), touched, len(tset)
