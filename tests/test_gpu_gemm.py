"""vr_gemm / vr_gemm_group against the float64 contract of tests/gemm_ref64.py: per-element derived bounds on every kernel family
(lean loop gemm_ntk.hip with every tile / ring / K-split share, gemm_nt.hip, the general kernel gemm.hip, the panel-resident kernel,
gemm_tn.hip and its group launches), at the tile, slice-ring and mask edges; exact probes (bound 0, torch.equal) for structure and for
the library's own grid-size rules; NaN canaries of a fixed bit pattern around everything a launch must not write and NaN in every
operand column it must not read; planted non-finite values; GELU at its edges.  Every launch is a valid call that must return VR_OK
(vitres.kernels raises otherwise).  The float64 reference of a case is computed once and shared by all its launches.

`pytest -s` prints one line per case (GEMM ...) and, last, the worst error / bound per form and family."""
import pytest
import torch

import gemm_ref64 as G
import vitres.kernels as K

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
IDS = {F32: "f32", BF16: "bf16", F16: "f16"}
SPECS = {s["name"]: s for s in G.fwd_specs()}
WSPECS = {s["name"]: s for s in G.wgrad_specs()}
LEAN_FORMS = {"plain", "bias", "bias_resid", "bias_resid_alias", "bias_resid_scale", "gelu_dual", "gelu_single", "gelu_pair", "dgrad",
              "dgrad_dact_saved"}
PANEL_BITS = [("panel", 0x200000), ("panel80", 0x200000 | 0x800000)]
WORST = {}
_CASES = {}


def case_ref(spec, dt, exact=False):
    """(case, float64 reference) of a forward case, built once; the device copies of its operands ride along"""
    key = (spec["name"], dt, exact)
    if key not in _CASES:
        c = G.build_fwd(spec, dt, exact=exact)
        if c is None:
            _CASES[key] = (None, None)
        else:
            c["dev"] = G.launch_buffers(c, DEV)
            _CASES[key] = (c, G.gemm64(c["a"], c["b"], c["kw"]))
    return _CASES[key]


def launch(c, **how):
    """one vr_gemm launch on fresh canary-filled outputs -> (out, out2, kw)"""
    a, b, out0, out20, kw = c["dev"]
    out, kw = out0.clone(), dict(kw)
    if c.get("resid_alias"):
        kw["resid"] = out
    if out20 is not None:
        kw["out2"] = out20.clone()
    K.gemm(a, b, out, **kw, **how)                          # raises unless VR_OK
    torch.cuda.synchronize()
    return out, kw.get("out2"), kw


def ratio_of(c, ref, out, out2, kw, shares=1):
    assert G.canary_intact(out, kw) and (out2 is None or G.canary_intact(out2, kw)), "wrote outside its output"
    r = G.nonfinite_ratio(G.logical(out, kw), ref["C"], G.bounds_for(ref, "C", shares))
    if out2 is not None:
        r = max(r, G.nonfinite_ratio(G.logical(out2, kw), ref["C2"], G.bounds_for(ref, "C2", shares)))
    return r


def note(form, family, r):
    WORST[(form, family)] = max(WORST.get((form, family), 0.0), r)


def lean_ok(spec, c):
    kw = c["kw"]
    return (c["a"].dtype != F32 and spec["form"] in LEAN_FORMS and kw["K"] % 64 == 0 and 64 <= kw["K"] <= 4096 and kw["N"] % 8 == 0
            and kw["ldc"] % 8 == 0 and kw.get("k_period", 0) in (0, 64, 128))


def panel_ok(spec, c):
    """what vr_gemm_panel_launch covers; anything else it hands on to the tiled kernels without a word, so this stays in step by hand"""
    kw = c["kw"]
    return (c["a"].dtype == BF16 and kw["out_dtype"] == BF16 and spec["form"] in G.PANEL_FORMS and kw["K"] % 32 == 0 and 32 <= kw["K"] <= 320
            and kw["N"] % 8 == 0 and kw["ldc"] % 8 == 0 and kw.get("k_period", 0) == 0 and not kw.get("a_map") and not kw.get("c_map"))


def families(spec, c):
    """[(label, family, launch keywords)]: every kernel family that takes the case, reached deliberately"""
    if c["a"].dtype == F32:
        return [("auto", "general-f32", {}), ("sched1", "general-f32", dict(sched=1))]
    fam = [("auto", "auto", {}), ("nt", "gemm_nt", dict(sched=0x100)), ("general", "general-16", dict(sched=4))]
    if lean_ok(spec, c):
        for tile in (1, 2, 3):
            for ring in (1, 2, 3, 4 if tile == 1 else 6):
                fam.append(("lean t%d r%d" % (tile, ring), "lean", dict(sched=tile << 11, ring=ring)))
    if panel_ok(spec, c):                                   # 144 rows x 8 waves up to K = 256, 80 rows x 4 waves; never its measurement bits
        fam += [(label, "panel", dict(sched=bits)) for label, bits in PANEL_BITS]
    return fam


def run_families(spec, dt, exact=False, fams=None):
    c, ref = case_ref(spec, dt, exact)
    if c is None:
        return
    rows = []
    for label, family, how in (fams or families(spec, c)):
        out, out2, kw = launch(c, **how)
        if exact:
            assert G.canary_intact(out, kw)
            assert torch.equal(G.logical(out, kw).cpu(), G.round_out(ref["C"], out.dtype)), (spec["name"], IDS[dt], label)
            continue
        r = ratio_of(c, ref, out, out2, kw)
        rows.append("%s=%.3f" % (label, r))
        note(spec["form"], family, r)
        assert r <= 1.0, (spec["name"], IDS[dt], label, r)
    print("GEMM %s %s%s: %s" % (spec["name"], IDS[dt], " exact" if exact else "", " ".join(rows) or "bit for bit"))


# ---- forward / data gradient: every shape x form x type on every family -------------------------------------------------------------------
@pytest.mark.parametrize("dt", G.DTYPES, ids=IDS.get)
@pytest.mark.parametrize("shape", G.FWD_SHAPES, ids=lambda s: "M%dN%dK%d" % s)
def test_forward_random(shape, dt):
    for form in G.FORMS:
        run_families(SPECS["%s-M%dN%dK%d" % ((form,) + shape)], dt)


@pytest.mark.parametrize("dt", G.DTYPES, ids=IDS.get)
@pytest.mark.parametrize("shape", G.FWD_SHAPES, ids=lambda s: "M%dN%dK%d" % s)
def test_forward_exact_probes(shape, dt):
    for form in G.EXACT_FORMS:
        run_families(SPECS["%s-M%dN%dK%d" % ((form,) + shape)], dt, exact=True)


@pytest.mark.parametrize("dt", G.DTYPES, ids=IDS.get)
@pytest.mark.parametrize("form", ["plain", "pos", "dgrad"])
def test_row_maps(form, dt):
    """A rows gathered through a_map, output rows scattered through c_map into a taller canary-filled buffer; unmapped A rows hold NaN"""
    run_families(SPECS["%s-maps-M66N72K128" % form], dt)
    run_families(SPECS["%s-maps-M66N72K128" % form], dt, exact=True)


@pytest.mark.parametrize("dt", [BF16, F16], ids=IDS.get)
def test_store_rounds_to_nearest_even(dt):
    """exact integer results where every odd one is a tie of the output type: a truncating or half-away store differs in the bits"""
    spec = dict(name="round-probe", form="bias", M=65, N=72, K=128, pad_c=True, pad_a=False)
    c = G.build_fwd(spec, dt, exact=True)
    c["kw"]["bias"] = c["kw"]["bias"] + G.ROUND_PROBE_OFFSET[dt]
    c["dev"] = G.launch_buffers(c, DEV)
    want = G.round_out(G.gemm64(c["a"], c["b"], c["kw"])["C"], dt)
    assert int((want.float() % 2 == 0).sum()) == want.numel() and float(want.float().abs().min()) > 128
    for label, _, how in families(spec, c):
        out, _, kw = launch(c, **how)
        assert torch.equal(G.logical(out, kw).cpu(), want), label


def test_fp16_overflows_to_infinity_as_common_h_states():
    spec = dict(name="f16-overflow", form="bias", M=65, N=72, K=128, pad_c=True, pad_a=False)
    c = G.build_fwd(spec, F16, exact=True)
    c["kw"]["bias"][::7] += 70000.0
    c["kw"]["bias"][3::7] -= 70000.0
    c["dev"] = G.launch_buffers(c, DEV)
    want = G.round_out(G.gemm64(c["a"], c["b"], c["kw"])["C"], F16)
    assert bool(torch.isinf(want).any()) and bool(torch.isfinite(want).any())
    for label, _, how in families(spec, c):
        out, _, kw = launch(c, **how)
        assert torch.equal(G.logical(out, kw).cpu(), want), label


def test_fp16_has_no_backward_forms():
    c, _ = case_ref(SPECS["plain-M65N72K128"], F16)
    a, b, out, _, kw = c["dev"]
    bt = torch.zeros(128, 72, dtype=F16, device=DEV)
    with pytest.raises(RuntimeError, match="VR_EUNSUPPORTED"):
        K.gemm(a, bt, out.clone(), **dict(kw, b_trans=True, ldb=72))


# ---- K-split shares ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(129, 136, 256), (193, 200, 512), (64, 264, 4096)], ids=lambda s: "M%dN%dK%d" % s)
def test_k_shares(shape):
    """2 - 4 workgroups share a tile's slices and meet in the role's workspace; at K = 256 (4 slices) the launcher clamps 3 and 4 shares to
    slices / 2.  The bound carries (shares - 1) u32 S for the shares the launcher clamps to (G.lean_shares; every form, tile and ring
    here has a split kernel and the workspace holds the slabs).  Afterwards the tickets are back at zero."""
    ws = K._workspace(torch.device(DEV))
    assert ws is not None
    for form in ("plain", "bias", "bias_resid_scale", "gelu_dual", "gelu_pair", "dgrad", "dgrad_dact_saved"):
        spec = SPECS["%s-M%dN%dK%d" % ((form,) + shape)]
        for exact in ((False, True) if form in G.EXACT_FORMS else (False,)):
            c, ref = case_ref(spec, BF16, exact)
            rows = []
            for tile in (1, 2, 3):
                for ring in (1, 3):
                    for shares in (2, 3, 4):
                        out, out2, kw = launch(c, sched=tile << 11, ring=ring, k_shares=shares, ws=ws)
                        if exact:
                            assert torch.equal(G.logical(out, kw).cpu(), G.round_out(ref["C"], out.dtype)), (form, tile, ring, shares)
                            continue
                        r = ratio_of(c, ref, out, out2, kw, G.lean_shares(shape[2], shares))
                        rows.append("t%dr%ds%d=%.3f" % (tile, ring, shares, r))
                        note(form, "lean+shares", r)
                        assert r <= 1.0, (spec["name"], tile, ring, shares, r)
            print("GEMM shares %s%s: %s" % (spec["name"], " exact" if exact else "", " ".join(rows) or "bit for bit"))
    assert int(ws[:16384].view(torch.int32).abs().sum()) == 0


# ---- the panel-resident kernel -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [0x200000, 0x200000 | 0x800000], ids=["panel", "panel80"])
@pytest.mark.parametrize("shape", [(63, 64, 64), (65, 72, 128), (127, 128, 192), (129, 136, 256)], ids=lambda s: "M%dN%dK%d" % s)
def test_panel_resident(shape, bits):
    """every form vr_gemm_panel_launch covers -- bias-less and bias store, GELU dual / single / pair, the saved-derivative multiply on a
    K-contiguous weight -- on both panel heights, random and exact.  (The panel kernel is also one of `families`: the mask, non-finite
    and GELU-edge tests run it too.)"""
    for form in G.PANEL_FORMS:
        spec = SPECS["%s-M%dN%dK%d" % ((form,) + shape)]
        assert panel_ok(spec, case_ref(spec, BF16)[0])
        run_families(spec, BF16, fams=[("panel", "panel", dict(sched=bits))])
        if form in G.EXACT_FORMS:
            run_families(spec, BF16, exact=True, fams=[("panel", "panel", dict(sched=bits))])


@pytest.mark.parametrize("form", G.PANEL_FORMS)
def test_panel_resident_beyond_its_144_row_form(form):
    """K in (256, 320]: only the 80-row / 4-wave form exists, with or without 0x800000"""
    spec = SPECS["%s-M129N136K320" % form]
    c, _ = case_ref(spec, BF16)
    assert panel_ok(spec, c)
    fams = [(label, "panel", dict(sched=bits)) for label, bits in PANEL_BITS]
    run_families(spec, BF16, fams=fams)
    if form in G.EXACT_FORMS:
        run_families(spec, BF16, exact=True, fams=fams)


# ---- masks ---------------------------------------------------------------------------------------------------------------------------------
MASK_NAMES = [n for n in SPECS if "-mask-" in n]


def _bits(t):
    return t.detach().cpu().contiguous().view(G.CANARY[t.dtype][0])


@pytest.mark.parametrize("dt", G.DTYPES, ids=IDS.get)
@pytest.mark.parametrize("name", MASK_NAMES)
def test_masks(name, dt):
    """keep_n / keep_k per sample with samples changing inside a tile, the -(k + 2) marker, periods, architecture groups 1 / 2 / 3 in the
    group-pure and the interleaved layout.  On every family: inside the bounds for every m_groups; the same launch without keep_k gives
    the identical bits (skipped slices are exact zeros)."""
    spec = SPECS[name]
    c, ref = case_ref(spec, dt)
    if c is None:
        return
    rows = []
    for label, family, how in families(spec, c):
        for mg in (1, 2, 3):
            out, out2, kw = launch(c, m_groups=mg, **how)
            r = ratio_of(c, ref, out, out2, kw)
            rows.append("%s g%d=%.3f" % (label, mg, r))
            note(spec["form"] + "+mask", family, r)
            assert r <= 1.0, (name, IDS[dt], label, mg, r)
            if mg == 1 or label in ("auto", "lean t2 r2", "lean t3 r1"):
                a, b, out0, out20, kwd = c["dev"]
                dense, kw2 = out0.clone(), {k: v for k, v in kwd.items() if k != "keep_k"}         # (k_period stays: the same kernel)
                if c.get("resid_alias"):
                    kw2["resid"] = dense
                if out20 is not None:
                    kw2["out2"] = out20.clone()
                K.gemm(a, b, dense, m_groups=mg, **kw2, **how)
                torch.cuda.synchronize()
                assert torch.equal(_bits(dense), _bits(out)), (name, IDS[dt], label, mg, "keep_k changed the bits")
                if out2 is not None:
                    assert torch.equal(_bits(kw2["out2"]), _bits(out2))
    print("GEMM %s %s: %s" % (name, IDS[dt], " ".join(rows)))


@pytest.mark.parametrize("tile", [0, 1, 2, 3])
@pytest.mark.parametrize("name", ["bias-mask-M136N136K192", "gelu_pair-mask-M136N136K192", "dgrad-mask-M136N136K192",
                                  "bias-mask-M136N192K256-periods"])
def test_masked_tiles_may_stay_unwritten(name, tile):
    """sched | 0x40000 (the caller vouches for its readers): kept columns inside their bounds; an element the contract masks holds +0 or
    the canary's bits, nothing else"""
    spec = SPECS[name]
    c, ref = case_ref(spec, BF16)
    it, cbits = G.CANARY[BF16]
    for mg in (1, 2):
        out, out2, kw = launch(c, m_groups=mg, sched=(tile << 11) | 0x40000)
        assert G.canary_intact(out, kw)
        for buf, val, bnd in ((out, ref["C"], ref["bC"]),) + (((out2, ref["C2"], ref["bC2"]),) if out2 is not None else ()):
            got = G.logical(buf, kw).cpu()
            masked = ~G.kept_mask(c["kw"]["keep_n"], kw["M"], kw["N"], kw["rows_in"], kw.get("n_period", 0))
            left = (got.view(it) == cbits) & masked
            assert not bool(((got.view(it) == cbits) & ~masked).any()), "a kept element was left unwritten"
            assert bool((got.view(it)[masked & ~left] == 0).all()), "a masked element holds something else than +0 or the canary"
            z = torch.zeros_like(val)
            r = G.worst_ratio(torch.where(left, torch.zeros((), dtype=BF16), got), torch.where(left, z, val), torch.where(left, z, bnd))
            note(spec["form"] + "+mask", "write-skip", r)
            assert r <= 1.0, (name, tile, mg, r)


# ---- non-finite values and GELU's edges ----------------------------------------------------------------------------------------------------
NF_SPECS = {form: dict(name="nf-%s" % form, form=form, M=68, N=72, K=128, pad_c=True, pad_a=False, rows_in=17, keep_n=[72, 40, 72, 8])
            for form in ("plain", "bias_resid_scale", "dgrad_dact_erf", "dgrad_dact_saved", "dgradk_dact_erf", "dgradk_dact_saved")}
PLANTS = {"plain": ["a", "b"], "bias_resid_scale": ["a", "b", "bias", "resid"], "dgrad_dact_erf": ["a", "dact_u"], "dgrad_dact_saved": ["dact_u"],
          "dgradk_dact_erf": ["dact_u"], "dgradk_dact_saved": ["a", "b", "dact_u"]}


@pytest.mark.parametrize("dt", G.DTYPES, ids=IDS.get)
@pytest.mark.parametrize("form", sorted(NF_SPECS))
def test_planted_non_finite_values(form, dt):
    """one NaN / +inf / -inf in an element of A, B, bias, resid or dact_u: NaN / inf in exactly the elements where the contract is, inside the
    bound elsewhere; a masked column stays an exact 0; sample 1 has scale 0 and keeps its NaN (the contract multiplies)"""
    spec = NF_SPECS[form]
    if not G.form_ok(form, dt):
        return
    for where in PLANTS[form]:
        for value in (float("nan"), float("inf"), float("-inf")):
            for m, n in ((20, 5), (20, 50), (3, 71), (60, 9)):       # (sample 1: scale 0, kept / masked), (sample 0), (sample 3: masked)
                c = G.build_fwd(spec, dt)
                kw = c["kw"]
                if where == "a":
                    c["a"][m, 7] = value
                elif where == "b":
                    (c["b"][7, n:n + 1] if kw["b_trans"] else c["b"][n, 7:8]).fill_(value)
                elif where == "bias":
                    kw["bias"][n] = value
                else:
                    kw[where][m, n] = value
                ref = G.gemm64(c["a"], c["b"], kw)
                assert not bool(torch.isfinite(ref["C"]).all()) or where != "a"
                masked = ~G.kept_mask(kw["keep_n"], 68, 72, 17, 0)
                if where != "resid":
                    assert bool((ref["C"][masked] == (G.f64(kw["resid"])[:68, :72][masked] if "resid" in kw else 0)).all())
                c["dev"] = G.launch_buffers(c, DEV)
                for label, family, how in families(spec, c):
                    out, out2, kwd = launch(c, **how)
                    r = ratio_of(c, ref, out, out2, kwd)
                    note(form + "+nonfinite", family, r)
                    assert r <= 1.0, (form, IDS[dt], where, value, (m, n), label, r)


GELU_U = [float("nan"), float("inf"), float("-inf"), 40.0, -40.0, 27.0, -27.0, 12.5, -12.5, 9.0, -9.0, 6.0, -6.0, 5.0, -5.0, 3.5, -3.5, 2.0, -2.0,
          1.0, -1.0, 0.75, -0.75, 0.25, -0.25, 2.0 ** -10, -2.0 ** -10, 2.0 ** -30, 0.0, -0.0, 0.7071, -0.7071]


@pytest.mark.parametrize("dt", G.DTYPES, ids=IDS.get)
@pytest.mark.parametrize("form", ["gelu_dual", "gelu_single", "gelu_pair", "dgrad_dact_erf", "dgradk_dact_erf"])
def test_gelu_at_its_edges(form, dt):
    """u is handed over exactly -- as the bias over a zero product, or as dact_u under a product of exactly 1 -- so the bound is the
    evaluation error of gelu / gelu' alone.  The float64 formulas give gelu(NaN) = gelu'(NaN) = NaN, gelu(+inf) = +inf,
    gelu(-inf) = NaN (-inf * 0), gelu'(+-inf) = NaN (inf * 0), and ordinary values for finite |u| up to 40: both implementations
    (erff for fp32, Abramowitz-Stegun for the 16-bit types) are held to them."""
    if not G.form_ok(form, dt):
        return
    spec = dict(name="gelu-edges-%s" % form, form=form, M=65, N=72, K=64, pad_c=True, pad_a=False)
    c = G.build_fwd(spec, dt, exact=True)
    kw = c["kw"]
    u = torch.tensor([GELU_U[i % len(GELU_U)] for i in range(72)], dtype=F32).to(dt)
    c["a"][:, :64] = 0
    if form.endswith("dact_erf"):
        c["a"][:, 0] = 1
        if kw["b_trans"]:
            c["b"][:, :72] = 0
            c["b"][0, :72] = 1
        else:
            c["b"][:, :64] = 0
            c["b"][:, 0] = 1
        kw["dact_u"][:65, :72] = u.view(1, 72)
    else:
        kw["bias"] = u.to(F32)
    ref = G.gemm64(c["a"], c["b"], kw)
    g_inf = ref["C2"] if "C2" in ref else ref["C"]
    if not form.endswith("dact_erf"):
        assert bool(torch.isnan(g_inf[0, 0])) and float(g_inf[0, 1]) == float("inf") and bool(torch.isnan(g_inf[0, 2]))
        assert abs(float(g_inf[0, 3]) - 40.0) < 1e-12 and abs(float(g_inf[0, 4])) < 1e-300
    c["dev"] = G.launch_buffers(c, DEV)
    rows = []
    for label, family, how in families(spec, c):
        out, out2, kwd = launch(c, **how)
        r = ratio_of(c, ref, out, out2, kwd)
        rows.append("%s=%.3f" % (label, r))
        note(form + "+edges", family, r)
        assert r <= 1.0, (form, IDS[dt], label, r)
    print("GEMM gelu edges %s %s: %s" % (form, IDS[dt], " ".join(rows)))


# ---- weight gradients ------------------------------------------------------------------------------------------------------------------------
def wgrad_launch(c, atomic, before, bias_grad=True, **how):
    a, b, out, _, kw = G.launch_buffers(c, DEV, atomic=atomic, before=before)
    M = kw["M"]
    bg = None
    if bias_grad:
        bg = (c["bg_before"].clone() if before == "rand" else (torch.zeros(M) if before == "zero" else torch.full((M,), G.NAN))).to(DEV)
    K.gemm(a, b, out, bias_grad=bg, **kw, **how)
    torch.cuda.synchronize()
    return out, bg, kw


def wgrad_ref(c, atomic, before, cache={}):
    key = (c["spec"]["name"], c["a"].dtype, c["exact"], atomic if atomic == 2 else before)
    if key not in cache:
        z = before != "rand" or atomic == 2
        cache[key] = G.gemm64(c["a"], c["b"], dict(c["kw"], atomic=atomic, bias_grad=True),
                              before=torch.zeros_like(c["before"]) if z else c["before"],
                              bias_grad_before=torch.zeros_like(c["bg_before"]) if z else c["bg_before"])
    return cache[key]


def wgrad_check(c, ref, out, bg, kw, split, tag):
    assert G.canary_intact(out, kw), tag
    got = G.logical(out, kw)
    if c["exact"]:
        assert torch.equal(got.cpu().double(), ref["C"]) and (bg is None or torch.equal(bg.cpu().double(), ref["bias_grad"])), tag
        return 0.0
    r = G.worst_ratio(got, ref["C"], G.bounds_for(ref, "C", split=split))
    if bg is not None:
        r = max(r, G.worst_ratio(bg, ref["bias_grad"], G.bounds_for(ref, "bias_grad", split=split)))
    assert r <= 1.0, (tag, r)
    return r


@pytest.mark.parametrize("dt", [F32, BF16], ids=IDS.get)
@pytest.mark.parametrize("name", sorted(WSPECS))
def test_wgrad(name, dt):
    """gemm_tn.hip (bf16, 8-element leading dimensions) and the general kernel (fp32; bf16 with No = 10): explicit splits 1, 2, 3, 7 and one
    more than there are 64-token slices (a split without tokens), atomic = 1 onto a non-zero `before` and onto zeros, atomic = 2 onto NaN
    (masked tiles included), bias_grad in both modes, row maps, token-sample keeps with 1 / 2 / 3 architecture groups"""
    spec = WSPECS[name]
    slices = (spec["T"] + 63) // 64
    groups = (1, 2, 3, 4) if spec.get("keep_k") else (0,)
    rows = []
    for exact in (False, True):
        c = G.build_wgrad(spec, dt, exact=exact)
        for mg in groups:
            for split in sorted({1, 2, 3, 7, slices + 1}):
                for before in ("rand", "zero"):
                    ref = wgrad_ref(c, 1, before)
                    out, bg, kw = wgrad_launch(c, 1, before, split_k=split, m_groups=mg)
                    # the launchers round a split to a multiple of the group count (group_split): bound with what can have run
                    used = max(split, G.group_split(split, spec["T"], mg))
                    r = wgrad_check(c, ref, out, bg, kw, used, (name, IDS[dt], exact, mg, split, before))
                    if spec.get("keep_k") and before == "rand":      # rows / columns beyond every keep: untouched, bit for bit
                        zr = G.wgrad_zero_region(spec)
                        assert torch.equal(G.logical(out, kw).cpu()[zr], c["before"][zr])
                    if not exact:
                        rows.append("s%d%s=%.3f" % (split, before[0], r))
                        note("wgrad" + ("+mask" if spec.get("keep_k") else ""), "tn" if (dt == BF16 and spec["No"] % 8 == 0) else "general-wgrad", r)
            if dt == BF16 and spec["No"] % 8 == 0:                   # the store form exists on gemm_tn.hip only
                ref = wgrad_ref(c, 2, "nan")
                out, bg, kw = wgrad_launch(c, 2, "nan", split_k=1, m_groups=mg)
                r = wgrad_check(c, ref, out, bg, kw, 0, (name, IDS[dt], exact, mg, "store"))
                if spec.get("keep_k"):
                    assert not bool((G.logical(out, kw).cpu()[G.wgrad_zero_region(spec)] != 0).any())
                if not exact:
                    rows.append("store=%.3f" % r)
                    note("wgrad-store", "tn", r)
    print("GEMM %s %s: %s" % (name, IDS[dt], " ".join(rows)))


def test_wgrad_store_form_exists_on_the_bf16_kernel_only():
    c = G.build_wgrad(WSPECS["wgrad-No64Ki64T63"], F32)
    with pytest.raises(RuntimeError, match="VR_EUNSUPPORTED"):
        wgrad_launch(c, 2, "nan", split_k=1)


@pytest.mark.parametrize("sched", [0, 64, 128, 0x10000])
@pytest.mark.parametrize("mode", ["atomic", "store", "mixed"])
@pytest.mark.parametrize("count", [2, 3, 4])
def test_wgrad_group(count, mode, sched):
    """vr_gemm_group with 2 - 4 problems of one T: every problem inside its own bounds and its own exact probe; store-form problems equal
    the one-by-one launch bit for bit (their order is fixed)"""
    T = 390
    dims = [(200, 328), (72, 136), (128, 128), (136, 264)][:count]
    for exact in (False, True):
        cases, calls, outs = [], [], []
        for i, (No, Ki) in enumerate(dims):
            atomic = 1 if mode == "atomic" else (2 if mode == "store" else 1 + i % 2)
            spec = dict(name="group-%d-No%dKi%dT%d" % (i, No, Ki, T), No=No, Ki=Ki, T=T, pad_c=i % 2 == 1)
            c = G.build_wgrad(spec, BF16, exact=exact)
            before = "rand" if atomic == 1 else "nan"
            a, b, out, _, kw = G.launch_buffers(c, DEV, atomic=atomic, before=before)
            bg = (c["bg_before"].clone() if atomic == 1 else torch.full((No,), G.NAN)).to(DEV)
            kw.update(bias_grad=bg, split_k=0, sched=sched if i == 0 else 0)
            cases.append((c, atomic, before))
            calls.append((a, b, out, kw))
            outs.append((out, bg, kw))
        K.gemm_group(calls)
        torch.cuda.synchronize()
        splits = G.tn_group_splits(dims, T, _cus(), [atomic for _, atomic, _ in cases], sched)      # the group's own rule, restated
        for (c, atomic, before), (out, bg, kw), split in zip(cases, outs, splits):
            ref = wgrad_ref(c, atomic, before)
            r = wgrad_check(c, ref, out, bg, kw, split if atomic == 1 else 0, (count, mode, sched, c["spec"]["name"], exact))
            note("wgrad-group", "tn-group", r)
            if atomic == 2:
                o1, b1, _ = wgrad_launch(c, 2, "nan", split_k=1)
                assert torch.equal(_bits(o1), _bits(out)) and torch.equal(_bits(b1), _bits(bg))


@pytest.mark.parametrize("sched", [0, 64, 128, 0x10000])
def test_wgrad_group_sums_the_bias_gradient_of_samples_that_keep_no_column(sched):
    """The training step's weight gradients run as groups: tn8_body (4 waves by default, 8 under 0x10000), tn_body under 64.  Token samples
    of 65 tokens with their own keeps.  Problem 0: EVERY sample keeps no column (a layer whose input width is 0) while its dY rows are
    kept -- whatever the split, each token range holds only such samples: C stays as it was, bit for bit, and bias_grad still sums every
    token.  Problem 1: samples 3 - 5 keep no column -- all of the second token range when the 8-wave kernel splits in two (tokens 256 ..
    389), part of the only range otherwise.  bias_grad and C against the float64 contract and the exact probe."""
    T = 390
    specs = [dict(name="group-nocols-all", No=72, Ki=136, T=T, pad_c=True, rows_in=65, keep_k=[72, 8, 64, 40, 0, 71], keep_n=[0] * 6),
             dict(name="group-nocols-tail", No=136, Ki=264, T=T, pad_c=False, rows_in=65, keep_k=[136, 8, 64, 129, 0, 135],
                  keep_n=[264, 129, 9, 0, 0, 0])]
    splits = G.tn_group_splits([(s["No"], s["Ki"]) for s in specs], T, _cus(), [1, 1], sched)
    for exact in (False, True):
        cases, calls, outs = [], [], []
        for i, spec in enumerate(specs):
            c = G.build_wgrad(spec, BF16, exact=exact)
            a, b, out, _, kw = G.launch_buffers(c, DEV, atomic=1, before="rand")
            bg = c["bg_before"].clone().to(DEV)
            kw.update(bias_grad=bg, split_k=0, sched=sched if i == 0 else 0)
            cases.append(c)
            calls.append((a, b, out, kw))
            outs.append((out, bg, kw))
        K.gemm_group(calls)
        torch.cuda.synchronize()
        for c, (out, bg, kw), split in zip(cases, outs, splits):
            ref = wgrad_ref(c, 1, "rand")
            assert bool((ref["bias_grad"] != ref["bg_before"]).any())
            r = wgrad_check(c, ref, out, bg, kw, split, (sched, c["spec"]["name"], exact))
            zr = G.wgrad_zero_region(c["spec"])
            assert torch.equal(G.logical(out, kw).cpu()[zr], c["before"][zr])
            note("wgrad-group+mask", "tn-group", r)


# ---- the library's own rules, at grid sizes that change them (exact probes, float32 reference) -------------------------------------------
def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _exact_big(spec, dt, fwd=True):
    c = (G.build_fwd if fwd else G.build_wgrad)(spec, dt, exact=True)
    A, B = (t.to(F32) for t in G.operands64(c["a"].float(), c["b"].float(), dict(c["kw"])))
    return c, A @ B.t()                                                                 # integers below 2^24: exact in fp32


def test_rule_picks_the_128_tile_on_a_full_grid():
    cu = _cus()
    tm = (2 * cu + 15) // 16
    spec = dict(name="rule-t128", form="bias", M=128 * tm - 3, N=2048, K=64, pad_c=False, pad_a=False)
    assert ((spec["M"] + 127) // 128) * 16 >= 2 * cu
    c, acc = _exact_big(spec, BF16)
    c["dev"] = G.launch_buffers(c, DEV)
    out, _, kw = launch(c)
    assert G.canary_intact(out, kw) and torch.equal(G.logical(out, kw).cpu(), (acc + c["kw"]["bias"]).to(BF16))


def test_persistent_workgroups_of_the_fp32_kernel_take_a_second_tile():
    cu = _cus()
    tm = (2 * cu + 5 + 7) // 8
    spec = dict(name="rule-persistent", form="bias_resid_alias", M=128 * tm - 5, N=1024 - 4, K=40, pad_c=True, pad_a=True)
    assert 2 * cu < tm * 8 <= 2 * cu + 16
    c, acc = _exact_big(spec, F32)
    c["dev"] = G.launch_buffers(c, DEV)
    out, _, kw = launch(c)
    want = acc + c["kw"]["bias"] + c["kw"]["resid"][:spec["M"], :spec["N"]]
    assert G.canary_intact(out, kw) and torch.equal(G.logical(out, kw).cpu(), want)


def test_by_fill_caps_the_token_split():
    cu = _cus()
    by_fill = (4 * cu + 255) // 256
    T = 64 * 32 * by_fill + 64
    assert (((T + 63) // 64) + 31) // 32 > by_fill == G.tn_split(2048, 2048, T, cu)
    spec = dict(name="rule-by-fill", No=2048, Ki=2048, T=T, pad_c=False)
    c, acc = _exact_big(spec, BF16, fwd=False)
    out, bg, kw = wgrad_launch(c, 1, "rand", split_k=0)
    assert G.canary_intact(out, kw) and torch.equal(G.logical(out, kw).cpu(), c["before"] + acc)
    assert torch.equal(bg.cpu(), c["bg_before"] + G.operands64(c["a"].float(), c["b"].float(), dict(c["kw"]))[0].to(F32).sum(1))


def test_general_kernel_takes_its_256_tile_for_a_long_weight_gradient():
    """M, N >= 192 and big_tiles * (K / 512) >= 192: gemm.hip's 256 x 256 persistent tile"""
    T = 512 * 192
    assert G.general_split(200, 264, T) == (192, True)
    spec = dict(name="rule-big-tile", No=200, Ki=264, T=T, pad_c=True)
    c, acc = _exact_big(spec, F32, fwd=False)
    out, bg, kw = wgrad_launch(c, 1, "rand", split_k=0)
    assert G.canary_intact(out, kw) and torch.equal(G.logical(out, kw).cpu(), c["before"] + acc)
    # the tile's fp32 row sums, added atomically by its 192 token splits: integers too
    assert torch.equal(bg.cpu(), c["bg_before"] + G.operands64(c["a"].float(), c["b"].float(), dict(c["kw"]))[0].to(F32).sum(1))


def test_zz_worst_ratios():
    """printed last: the worst error / bound per form and kernel family of this run (DESIGN.md carries the table)"""
    for (form, family), r in sorted(WORST.items()):
        print("GEMM WORST %-28s %-14s %.3f" % (form, family, r))
    assert all(r <= 1.0 for r in WORST.values())
