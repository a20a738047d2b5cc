"""The conv GEMM kernels (csrc/kernels/convgemm.hip, conv_big.hip, conv_bwd_fused.hip) per element against
tests/conv_oracle.py, on every dispatch path.  native() entry points are called directly and every kernel
gets oracle inputs for what is upstream of it (coefficients, mean / invstd and bits are built on the CPU).

Bounds (the project's rules; conv_oracle's docstring has the rounding points and the ambiguity sets)
    bf16 outputs   no element outside |kernel - yardstick| <= 2^-6 |yardstick| + 2^-14 mag (+ ulp |b| for
                   staged values in set (b)); rowerr(kernel, exact) <= 3 rowerr(yardstick, exact)
    fp32 sums      every slab of part, and db, against fp64 sums of the kernel's OWN stored bf16 output:
                   |got - oracle| <= 2^-24 L sum |terms|, L from the plan replay; part.shape == [slabs, G, N]
    exact          abits == (aout > 0); masked elements are 0; epilogue 9 == epilogue 6 in c and its first two
                   slabs; impulse cases bit for bit; every output identical on a second call
The two-source prologues store their staged A (aout): it is judged by the BatchNorm rules, and the GEMM
oracle is then formed from the kernel's own aout.

Case -> kernel instantiation (each case asserts it before it runs: tile and grid through conv_gemm_plan, the
ladder branch through conv_gemm_family -- the value launch_conv_fwd itself branches on --, conv_wgrad_plan --
the plan launch_conv_wgrad itself consumes --, conv_dgrad_s2_plan, conv11_bwd_fused_supported; and each
against conv_oracle's replay)
    launch_conv_fwd
      reg          conv_fwd_kernel<128, 64|128, kProNone|kProBnRelu, EPI, KS1, GLDS=false>: 1x1 M in {1, 127, 129,
                   300} x K in {64, 128} x N in {64, 128, 192 (bn 64)}, epilogues 0-9, kProBnRelu with 0 / 1; 1x1
                   stride 2 on 13 x 11 (KS1 with the pixel decode); persistent (tpb = 3): 157 tiles / 64 blocks
                   (K 64, N 1024, M 20000) and 313 / 128 (K 128, N 512, M 40001), epilogues 1 3 6 9, kProBnRelu
                   at K 64 / 128 (resident weight tile, nk <= 2) and K 256 (nk = 4);
                   <128, 64|128, kProBnRelu, 0|1, KS1=false, false>: 3x3 on 7 x 5 and 9 x 9 (stride 1; 9 x 9 also
                   stride 2), C 64 / 128, N 64 / 128 / 192 -- a padded tap must stay 0 after the prologue
      twosrc_reg   <128, 64, kProBlockOut, 0|1, true, false> (the plan forces bn 64 for every N; M 20000:
                   157 tiles / 64 blocks) and <128, 64|128, kProBnBwd, 3, true, false> (N 128; N 64 / 192),
                   K in {64, 192}
      twosrc_glds  <128, 128, kProBlockOut, 0|1, true, true> and <128, 128, kProBnBwd, 3, true, true> (N 128),
                   <128, 64, kProBlockOut, 0|1, true, true> and <128, 64, kProBnBwd, 3, true, true> (N 64 / 192:
                   three stage buffers under the 128 x 68 output tile), K in {256, 512}
      glds         <128, 64|128, kProNone, EPI, KS1|!KS1, true>: K in {192, 512} epilogues 0-9; 3x3 C 128
                   strides 1 / 2 on 9 x 9, 7 x 5, 9 x 1, 2 x 2 (zero-page taps)
      tall         <256, 64, kProNone, EPI != 9, KS1|!KS1, true>: K 512 and 3x3 C 64, M in {255, 257, 600}
      patch        <128, 128, kProNone, 0|1|3, false, true, VAR=1>: 12 x 11, 9 x 15 (n = 3), 28 x 28 (n = 2)
      not reached  ONE_GLDS (kProBnRelu on the LDS-DMA path inside conv_fwd_body) is instantiated by no
                   launcher ladder: PSAMD_CF sends every prologue to GLDS=false.  The patch tiles with bn 64:
                   patch_fwd_ok needs N % 128 == 0.
      empty blocks every planner gives gm <= tiles (persistent: min(tiles, cap); else one block per tile; each
                   stride-2 phase: its own tile count, padding blocks of the merged grid return before they
                   write), so no binding can make a partial-sum row whose block owns no tile; the sum check
                   compares every row of part, so such a row would have to be exactly 0.
    launch_conv_big   conv_big_kernel<EPI, PRO> for all 22 pairs at M 65300, K 1024, N 256 (256 blocks, the last
                   tile 20 rows), and the stride-2 gather without prologue
    launch_conv_dgrad_phases   conv_dgrad_phases_kernel<64|128, 0|3> on 6 x 4, 14 x 10, 8 x 12
    launch_conv_wgrad
      narrow       conv_wgrad_kernel<1|2, 1|2, PRO, GL = !PRO>; 3x3; 1x1 stride 2; 1, 8 and 19 slabs (two levels)
      wide         conv_wgrad_wide_kernel<.., PRO, DB, LIN, PROL>, per instantiation:
                   no prologue   kinds 1 2 3 4 with LIN (1x1 stride 1); kind 1 (1x1 stride 2) and kind 4 (3x3,
                                 strides 1 / 2) without LIN
                   PROL          kinds 1 2 3 with LIN; kind 1 without (1x1 stride 2)
                   fragment prologue (tk 384)   kind 4 with LIN and without (1x1 stride 2, C 384)
                   DB            kinds 1 2 3 4 through linear_wgrad_db, LIN only: that binding always passes the
                                 [M, 1] geometry, and fc_bwd runs fc.hip's own kernel, not this one
                   kinds 2 / 3 without LIN and not-LIN PROL of kinds 2 / 3 differ from the rows above only in
                   the tile constants and are not run.  3 and 18 slabs (two levels; 512 x 512: one level, the
                   E >= 2^18 exception)
      patch        conv_wgrad_patch_kernel<56, 1>, <28, 1>, <56, 2> at one image
    conv11_bwd_fused  <64, 256, PLAIN = false|true>, M in {1, 129, 300, 33000 (258 tiles / 256 blocks)}

Observed on MI355X (test_zz_report prints these; pytest -rP).  Per family: the worst rowerr(kernel, exact) /
rowerr(yardstick, exact) with that yardstick's own rowerr in brackets, the worst share of the elementwise
bound, the worst share of a sum bound.  No bound is tuned to them; none is near its limit and none was widened
(the 2^-24 L fallback for long reductions was not needed).
    reg                1.000 (1.85e-03)   0.510   0.242        tall               1.000 (2.00e-03)   0.398   0.155
    glds               1.000 (1.92e-03)   0.415   0.195        patch              1.000 (2.00e-03)   0.435   0.180
    twosrc_reg         1.000 (1.84e-03)   0.487   0.264        twosrc_reg/aout    1.000 (2.26e-03)   0.449   -
    twosrc_glds        1.000 (1.97e-03)   0.395   0.246        twosrc_glds/aout   1.000 (1.94e-03)   0.494   -
    big                1.000 (2.12e-03)   0.729   0.213        big/aout           1.000 (1.88e-03)   0.498   -
    dgrad_s2/bn64      1.000 (1.92e-03)   0.000   0.131        dgrad_s2/bn128     1.000 (1.89e-03)   0.023   0.115
    wgrad/kind0        1.000 (2.08e-03)   0.406   -            wgrad/kind1        1.000 (1.82e-03)   0.408   -
    wgrad/kind2        1.000 (1.88e-03)   0.243   -            wgrad/kind3        1.000 (1.84e-03)   0.322   -
    wgrad/kind4        1.000 (1.75e-03)   0.237   -            wgrad/kind5        1.000 (1.76e-03)   0.396   -
    wgrad/kind1/db     1.000 (1.85e-03)   0.376   0.002        wgrad/kind2/db     1.000 (1.99e-03)   0.191   0.002
    wgrad/kind3/db     1.000 (1.78e-03)   0.159   0.002        wgrad/kind4/db     1.000 (1.76e-03)   0.401   0.002
    fused/bn2/gy       1.000 (1.08e-03)   0.452   0.065        fused/bn2/dw       1.000 (2.30e-03)   0.408   -
    fused/plain/gy     1.000 (1.15e-03)   0.465   -            fused/plain/dw     1.000 (2.24e-03)   0.252   -
The row ratio is 1.000 everywhere because the final bf16 rounding, which kernel and yardstick share,
dominates both errors; the fp32 accumulation adds < 1e-3 of it.

Found by this file: epilogue 9 on 64-channel tiles (N % 128 != 0) kept its third running sum in LDS slots
that lie inside stage buffer A1 (the 128 x 68 output tile ends before the stage buffers do), so the staging
writes of the next stage overwrote it: third slab off by 1e5-1e6 x its bound at K >= 128, M > 8.  The model
only runs epilogue 9 with N % 128 == 0; fixed in conv_fwd_body (S3_BASE), cases kept.
"""
import math

import pytest
import torch

from ps_amd.ops import native

from . import conv_oracle as co

pytestmark = pytest.mark.gpu
DEV = "cuda"
OPERANDS = ("aux", "kshift", "mc", "mean", "invstd", "bits", "aux2", "bits2", "a2", "bwd", "aux3", "mean2", "invstd2",
            "pro2")
STATS = {}  # family -> dict(ratio, yard, elem, sums): the worst figures seen, printed by test_zz_report
_ACC = {}   # operand set -> (aout, acc, mag): the GEMM oracle over a kernel's own aout, shared by the epilogues


def _d(t):
    return None if t is None else t.to(DEV).contiguous()


def _judge(fam, got, o, extra=None, L=None):
    """The elementwise rule and the row rule for one bf16 output against oracle dict o."""
    got = got.double().cpu()
    mag = co.with_extra(o["mag"], extra, L)
    if o.get("amb") is not None and bool(o["amb"].any()):  # set (a): either masked value
        tol = co.REL * o["alt"].abs() + co.MAGREL * mag
        got = torch.where(o["amb"] & ((got - o["alt"]).abs() <= tol), o["yard"], got)
    bad, worst = co.elemerr(got, o["yard"], mag)
    ry, rk = co.rowerr(o["yard"], o["exact"]), co.rowerr(got, o["exact"])
    s = STATS.setdefault(fam, dict(ratio=0.0, yard=0.0, elem=0.0, sums=0.0))
    s["elem"] = max(s["elem"], worst)
    if ry > 0 and rk / ry > s["ratio"]:
        s["ratio"], s["yard"] = rk / ry, ry
    print(f"{fam}: elem bad {bad} worst {worst:.3f}; rowerr {rk:.3e} (yardstick {ry:.3e})")
    assert bad == 0, f"{bad} elements outside the rule (worst {worst:.2f} x)"
    assert rk <= 3.0 * ry, f"rowerr {rk:.3e} > 3 x {ry:.3e}"


def _judge_sums(fam, part, terms, blocks, G, L):
    """Every slab of part against fp64 block sums of the terms."""
    part = part.double().cpu()
    assert tuple(part.shape) == (len(terms), G, terms[0].shape[1]), part.shape
    assert bool(torch.isfinite(part).all())
    s, a = co.block_sums(terms, blocks, G)
    tol = co.U24 * L * a
    share = float(((part - s).abs() / tol.clamp_min(1e-300)).max()) if bool((tol > 0).any()) else 0.0
    st = STATS.setdefault(fam, dict(ratio=0.0, yard=0.0, elem=0.0, sums=0.0))
    st["sums"] = max(st["sums"], share)
    print(f"{fam}: sums worst share {share:.3f} of 2^-24 x {L} x sum|terms|")
    assert bool(((part - s).abs() <= tol).all()), f"a partial sum off by {share:.2f} x its bound"


def _conv_gemm(case, t, epi=None):
    kw = {k: _d(t[k]) for k in OPERANDS if t.get(k) is not None}
    a = _d(t["a"])
    aout = abits = None
    if case["pro"] == co.PRO_BLOCK_OUT:
        aout = torch.full_like(a, float("nan"))
        abits = torch.zeros(a.numel() // 8, dtype=torch.uint8, device=DEV)
        kw.update(aout=aout, abits=abits)
    e = case["epi"] if epi is None else epi
    if e == 6:
        for k in ("aux3", "mean2", "invstd2"):
            kw.pop(k, None)
    r = native().conv_gemm(a, _d(t["b"]), t["geo"], _d(t.get("pro")), e, **kw)
    torch.cuda.synchronize()
    if case["pro"] == co.PRO_BN_BWD:
        aout = r[2]
    part = r[1] if r[1] is not None and r[1].numel() else None
    return [None if x is None else x.cpu() for x in (r[0], part, aout, abits)]


def _same(u, v):
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(u, v))


def _run_fwd(case, device=None):
    nv = native()
    g = co.geo(case["H"], case["W"], case["ks"], case["stride"], case["pad"])
    M, N, C, pro, epi = case["images"] * g[2] * g[3], case["N"], case["C"], case["pro"], case["epi"]
    plan = co.plan_fwd(M, N, C, g, pro, epi)
    src2 = {co.PRO_BLOCK_OUT: 1, co.PRO_BN_BWD: 2}.get(pro, 0)
    assert list(nv.conv_gemm_plan(M, N, C, g, pro != 0, epi, src2)) == [plan["bm"], plan["bn"], plan["gm"]]
    assert (plan["family"], plan["tpb"]) == (case["family"], case["tpb"]), plan
    assert nv.conv_gemm_family(M, N, C, g, pro, epi) == co.FAMILY[plan["family"]]
    fam = plan["family"]
    t = co.fwd_inputs(case, device)
    assert t["share_a"] <= co.CAP and t["share_b"] <= co.CAP
    out = _conv_gemm(case, t)
    assert _same(out, _conv_gemm(case, t)), "a second call gave different bits"
    c, part, aout, abits = out
    acc, mag = t["acc"], t["mag"]
    if pro in (co.PRO_BLOCK_OUT, co.PRO_BN_BWD):  # the staged A by the BatchNorm rules, then the GEMM over it
        _judge(fam + "/aout", aout, dict(yard=t["aout_yard"], exact=t["aout_exact"], mag=t["aout_mag"]))
        if pro == co.PRO_BLOCK_OUT:
            assert torch.equal(abits, co.mask_bits(aout.double())), "abits != (aout > 0)"
        key = (co.case_id(dict(case, epi=0)), fam)
        hit = _ACC.get(key)
        if hit is None or not torch.equal(hit[0], aout):
            A, bt = aout.double(), t["b"].double().t()
            _ACC.clear()
            hit = _ACC[key] = (aout, co.mm(A, bt, device), co.mm(A.abs(), bt.abs(), device))
        acc, mag = hit[1], hit[2]
    o = co.epilogue(epi, acc, mag, t)
    if case.get("kind") == "impulse":
        assert torch.equal(c.view(torch.int16), t["A"][:, t["kn"]].bfloat16().view(torch.int16))
        return
    _judge(fam, c, o, t.get("extra"))
    cd = c.double()
    if epi == 3:
        assert bool((cd[~o["on"] & ~o["amb"]] == 0).all()), "a masked element is not 0"
    if epi >= 6:
        assert bool((cd[~co.unpack_bits(t["bits2"], (M, N))] == 0).all()), "an element masked by bits2 is not 0"
    terms = co.sum_terms(epi, c, t)
    if terms:
        _judge_sums(fam, part, terms, co.fwd_blocks(M, plan["bm"], plan["gm"]), plan["gm"], plan["L"])
    else:
        assert part is None
    if epi == 9:
        c6, p6, _, _ = _conv_gemm(case, t, 6)
        assert torch.equal(c6, c) and torch.equal(p6, part[:2]), "epilogue 9 differs from epilogue 6"


@pytest.mark.parametrize("case", co.FWD_CASES, ids=co.case_id)
def test_conv_gemm_rows(case):
    big = case["images"] * case["H"] * case["W"] >= 20000
    _run_fwd(case, DEV if big else None)


@pytest.mark.parametrize("case", co.BIG_CASES, ids=co.case_id)
def test_conv_big_rows(case):
    _run_fwd(case, DEV)


@pytest.mark.parametrize("images,H,W,C1,C2", co.DGRAD_S2_CASES)
@pytest.mark.parametrize("epi", [0, 3])
def test_conv_dgrad_s2_rows(images, H, W, C1, C2, epi):
    t = co.dgrad_s2_inputs(images, H, W, C1, C2, epi, 31 + H + C1 + epi)
    assert t["share_a"] <= co.CAP
    M = images * (H // 2) * (W // 2)
    bn, gm = native().conv_dgrad_s2_plan(M, C1)  # launch_conv_dgrad_phases: <BN, EPI>, one 128-pixel tile per block
    assert bn == (128 if C1 % 128 == 0 else 64)
    wph = [_d(co.phase_weight(t["w"], ph >> 1, ph & 1)) for ph in range(4)]

    def call():
        r = native().conv_dgrad_s2(_d(t["dz"]), wph, H, W, epi, _d(t.get("aux")), _d(t.get("mc")), _d(t.get("mean")),
                                   _d(t.get("invstd")))
        torch.cuda.synchronize()
        return [r[0].cpu(), r[1].cpu() if r[1] is not None and r[1].numel() else None]

    out = call()
    assert _same(out, call())
    o = co.dgrad_s2_oracle(t, images, H, W, epi)
    assert o["G"] == 4 * gm
    _judge(f"dgrad_s2/bn{bn}", out[0], o)
    if epi == 3:
        assert bool((out[0].double()[~o["on"] & ~o["amb"]] == 0).all())
        cpr = bn // 8
        L = 128 // (256 // cpr) + int(math.log2(64 // cpr)) + 2 + 3
        _judge_sums(f"dgrad_s2/bn{bn}", out[1], co.sum_terms(3, out[0], t), o["block"], o["G"], L)
    else:
        assert out[1] is None


def _wgrad_plan(M, N, K, C, g, pro):
    p = co.plan_wgrad(M, N, K, C, g, pro)
    assert list(native().conv_wgrad_plan(M, N, K, C, g, pro)) == [p[k] for k in ("kind", "tn", "tk", "tiles", "nsplit",
                                                                                  "rows", "groups")]
    return p


@pytest.mark.parametrize("case", co.WGRAD_CASES, ids=co.wgrad_id)
def test_conv_wgrad_rows(case):
    t = co.wgrad_inputs(case)
    assert t["share_b"] <= co.CAP
    g, M, N, C = t["geo"], t["M"], case["N"], case["C"]
    p = _wgrad_plan(M, N, case["ks"] ** 2 * C, C, g, case["pro"])
    assert (p["kind"], p["levels"]) == (case["wkind"], case["levels"]), p

    def call():
        r = native().conv_wgrad(_d(t["dz"]), _d(t["x"]), g, _d(t["pro"]))
        torch.cuda.synchronize()
        return r.cpu()

    dw = call()
    assert torch.equal(dw, call())
    o = co.wgrad_oracle(t["dz"], t["A"], None, t["amb"], t["ulp"])
    if case.get("kind") == "impulse":
        assert torch.equal(dw.view(torch.int16), t["A"][t["mn"]].bfloat16().view(torch.int16))
        return
    _judge(f"wgrad/kind{p['kind']}", dw, o, o["extra"])


@pytest.mark.parametrize("M,N,K,levels", co.DB_CASES)
def test_linear_wgrad_db_rows(M, N, K, levels):
    """The DB variant of the wide kernel: dW as above, db = column sums of dz in fp32."""
    g = [M, 1, M, 1, 1, 1, 0]
    p = _wgrad_plan(M, N, K, K, g, False)
    assert 1 <= p["kind"] <= 4 and p["levels"] == levels
    dz, x = co.db_inputs(M, N, K)

    def call():
        r = native().linear_wgrad_db(_d(dz), _d(x))
        torch.cuda.synchronize()
        return [r[0].cpu(), r[1].cpu()]

    dw, db = call()
    assert _same([dw, db], call())
    o = co.wgrad_oracle(dz, x.double())
    _judge(f"wgrad/kind{p['kind']}/db", dw, o)
    assert db.dtype == torch.float32 and tuple(db.shape) == (N,)
    share = float(((db.double() - o["db"]).abs() / (co.U24 * p["L_db"] * o["db_mag"])).max())
    st = STATS.setdefault(f"wgrad/kind{p['kind']}/db", dict(ratio=0.0, yard=0.0, elem=0.0, sums=0.0))
    st["sums"] = max(st["sums"], share)
    assert share <= 1.0, f"db off by {share:.2f} x 2^-24 x {p['L_db']} x sum |dz|"


@pytest.mark.parametrize("M", co.FUSED_MS)
@pytest.mark.parametrize("plain", [False, True])
def test_conv11_bwd_fused_rows(M, plain):
    assert native().conv11_bwd_fused_supported(64, 256, plain)
    p = co.plan_fused(M)
    t = co.fused_inputs(M, plain, 77 + M)

    def call():
        r = native().conv11_bwd_fused(_d(t["g"]), _d(t["z3"]), _d(t["cbwd"]), _d(t["wt"]), _d(t["z2"]), _d(t.get("cf2")),
                                      _d(t.get("mean2")), _d(t.get("invstd2")))
        torch.cuda.synchronize()
        return [x.cpu() for x in r]

    gy, part, dw = call()
    assert _same([gy, part, dw], call())
    o = co.fused_oracle(t, plain, DEV if M > 1000 else None)
    assert o["share_a"] <= co.CAP and o["share_b"] <= co.CAP
    fam = "fused/plain" if plain else "fused/bn2"
    _judge(fam + "/gy", gy, o["gy"], o["gy"]["extra"])
    _judge(fam + "/dw", dw, o["dw"], o["dw"]["extra"])
    if plain:
        assert tuple(part.shape) == (0, p["gm"], 64)
        return
    assert bool((gy.double()[~o["gy"]["on"] & ~o["gy"]["amb"]] == 0).all())
    terms = co.sum_terms(3, gy, dict(aux=t["z2"], mean=t["mean2"], invstd=t["invstd2"]))
    _judge_sums(fam, part, terms, co.fwd_blocks(M, 128, p["gm"]), p["gm"], p["L"])


def test_zz_report():
    """Prints the worst figures of this run per output family (pytest -rP shows them)."""
    for fam in sorted(STATS):
        s = STATS[fam]
        print(f"{fam:24s} rowerr ratio {s['ratio']:.3f} (yardstick {s['yard']:.2e})  elem {s['elem']:.3f}  sums {s['sums']:.3f}")
