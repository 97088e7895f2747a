"""The any-strides contract of every entry point that reads ensemble members
(include/eks_hip.h: obs[b*sb + t*st + e*se + j*sj], "strides in ELEMENTS, any
layout"): eks_ensemble, eks_smooth, eks_smooth_var, eks_nll_sweep,
eks_smooth_seg, eks_fit, and the gaps family eks_smooth_gaps,
eks_nll_sweep_gaps, eks_draws_gaps, eks_fit_gaps, eks_ensemble_gaps,
eks_fit_pupil -- and of the output strides of eks_smooth, eks_smooth_gaps
(pvar shares out's), eks_smooth_var and eks_draws_gaps.

The member views come from tests/layouts.py: each is carved out of a larger
allocation filled with poison, so a wrong address shows in the result, never
as a fault.  The poison is NaN where the entry point propagates NaN and a
finite 1e30 for the gaps family, whose inputs carry their own NaN members and
which is run in "mean" mode as well as "median" (one misread member moves a
mean by orders of magnitude) and compared on its integer outputs too.

    tm            (T,E,n,B) contiguous: canonical, every other layout is compared with it
    bm            (B,T,E,n) contiguous, 16-byte aligned base: vec, staged and packed true
    bm_off1       bm, base one element in: base alignment false, strides perfect
    bm_off2_f32   bm, base two float32 (8 bytes) in: half-aligned base
    bm_padT1      bm with st = E*n + 1: row stride no 16-byte multiple, vec and packed false
    bm_padT4      bm with st = E*n + 4: vec true, staged false; packed true
    bm_padB1      bm with sb = T*E*n + 1: packed's (sb*ts) % 16 false for B > 1
    coord_major   (B,T,n,E), se = 1, sj = E: sj != 1, vec and packed false
    member_outer  (E,B,T,n), se the largest stride: the reference's list of models, se != n
    t_inner       (B,E,n,T), st = 1: unit step stride
    tm_padB       (T,E,n,B+3), base one element in: ragged, offset trajectory axis
    shared_bm     sb = 0, one bm trajectory expanded: k_c0_shared with vec and staged true
    shared_off1   sb = 0, one bm_off1 trajectory expanded: k_c0_shared, vec false by the base
    shared_padT4  sb = 0, one bm_padT4 trajectory expanded: k_c0_shared, vec true, staged false
    shared_padT1  sb = 0, one bm_padT1 trajectory expanded: k_c0_shared, vec false by st alone
    shared_coord  sb = 0, one coord_major trajectory expanded: k_c0_shared, sj != 1 and se != n

Two comparisons per entry point:

(a) ``test_tm_*``: the result on ``tm`` against the CPU reference the suite
    already uses for that entry point, under that file's bound (imported, not
    restated).  At B = 70 the reference is computed for the trajectories
    ANCHOR_ROWS (the first two, both sides of the wave boundary, the last).
(b) ``test_layout_*``: every other layout's outputs equal the ``tm`` outputs
    BIT FOR BIT -- out, ms, nll, var, Vs, status, nobs, params, the hand-off
    planes, the statistics, the counts, the draws.  The layout changes where a
    member is fetched from, not which values are reduced, the lane-to-
    trajectory mapping or the algorithm (``pick_algo`` does not see strides;
    none of these layouts has the negative or > 2 GB strides that make
    ``smooth_call`` swap algo 3 for algo 2).  The partner of a ``shared``
    layout is its materialised copy (``.contiguous()`` of the expanded view).
    There eks_smooth's algo 2 moves the ensemble into k_c0_shared and hands y
    and ev on through planes; the planes hold the very doubles (or, for an
    odd-E float32 median, the very member value) that the member path reduces
    in registers, and test_fit_yev_handoff_bit_exact already holds plane input
    to the bits of member input, so these pairs are compared bit for bit too.

Which run-time branch a kernel took cannot be observed from outside.  Coverage
of ``vec``, ``staged`` and ``packed`` is by construction: every test asserts
``data_ptr() % 16`` and the four strides of the tensor it built against the
layout's claim and evaluates the kernels' predicates on them, and
test_layouts_host.py holds predicates and claims together on the CPU.

Shapes: T = 613 (more than two 256-step blocks of k_c0_shared; no multiple of
4, 64 or 256; 39 chunks of 16 in the time-parallel forms, asserted), B in
{1, 3, 70}, (r, n, E) in {(2,2,4), (2,2,5), (3,8,5)} and the runtime-n shape
(3,10,5) of test_gpu_rt.py.
"""
import functools
import warnings

import numpy as np
import pytest

import draws_ref as D
import ensemble_gaps_ref as R
import gaps_ref as G
import gaps_sweep_data as GS
import layouts as LY
import sweep_data as SD

pytestmark = pytest.mark.gpu

T = 613
SHAPES = {"sv4": (2, 2, 4), "sv5": (2, 2, 5), "mc": (3, 8, 5), "rt": (3, 10, 5)}
COMPILED = ("sv4", "sv5", "mc")
BS = (1, 3, 70)
DTYPES = [np.float32, np.float64]
SCALES = (0.1, 1.0, 10.0)  # the sweeps' candidates: Q x s
NDRAWS = 3
NSEG = 3
NAN, BIG = float("nan"), 1e30


def ANCHOR_ROWS(B):
    return list(range(B)) if B <= 3 else [0, 1, 63, 64, B - 1]


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


# ---------------------------------------------------------------------------
# the problems: members, gaps, models; computed once and shared, read only
# ---------------------------------------------------------------------------
def gap_mask(B, n, kind):
    """(B, T, n) the columns whose member 0 is NaN: random gaps (20 % single
    view, 3 % multi-camera: the fits need complete frames), trajectory 0 with
    a void across chunk boundaries, a camera out, the first and last frame."""
    frac = 0.2 if kind == "sv" else 0.03
    mask = np.random.default_rng(613 + 7 * B + n).random((B, T, n)) < frac
    mask[0, 200:260] = True
    mask[0, 300:380, 0:2] = True
    mask[0, 0] = True
    mask[0, -1] = True
    if B > 1:
        mask[1, 90:100] = True
        mask[1, -1, n - 1] = True
    if B > 2:
        mask[2] = False
    return mask


@functools.lru_cache(maxsize=None)
def problem(shape, B):
    r, n, E = SHAPES[shape]
    kind = "sv" if n == 2 else "mc"
    st = G.members(kind, B, T, V=n // 2, E=E)
    models = [G.model_of(kind, st[b]) for b in range(B)]
    g = G.knock_out(st, gap_mask(B, n, kind))
    gm = R.knock_members(st, R.member_mask(1000 * B + n + E, B, E, T, n, 0.30))
    gm[0, :, 5, :] = np.nan          # a frame with no valid member
    gm[0, 0, 7, 0] = np.inf
    gm[B - 1, E - 1, T - 1, n - 1] = -np.inf
    z = np.random.default_rng(5000 + B + n).standard_normal((B, NDRAWS, T, r))
    for a in (st, g, gm, z):
        a.setflags(write=False)
    return dict(shape=shape, r=r, n=n, E=E, B=B, kind=kind, st=st, g=g, gm=gm, z=z, models=models)


@functools.lru_cache(maxsize=None)
def shared_models(shape, B):
    """B candidate models of trajectory 0 (a shared layout repeats it)."""
    P = problem(shape, B)
    return [GS.scaled(P["models"][0], 10.0 ** (-1 + 2 * b / max(B - 1, 1))) for b in range(B)]


@functools.lru_cache(maxsize=None)
def pupil_problem(E, B):
    import test_gpu_fit_pupil as FP
    st = FP.members(B, T, E)
    g = FP.with_gaps(st, seed=E + B, blink=(100, 160), inf_at=300)
    g.setflags(write=False)
    return dict(shape=f"pupil{E}", r=3, n=8, E=E, B=B, kind="pupil", pupil=g)


def device_rows(torch, models, scales=(1.0,)):
    """(len(scales) * B, P) float64 CUDA rows: row k * B + b = models[b] with Q x scales[k]."""
    return torch.from_numpy(GS.rows_of([[GS.scaled(m, s) for m in models] for s in scales])).cuda()


def model_arrays(models):
    return np.stack([m["A"] for m in models]), np.stack([m["C"] for m in models])


# ---------------------------------------------------------------------------
# the entry points: (members view, problem, models, variant) -> dict of tensors
# ---------------------------------------------------------------------------
def yev_planes(torch, yev, out, key="yev"):
    """The y and ev planes of a hand-off (without the padding between them)."""
    from eks_amd import _lib
    B, T_, _, n = yev.shape
    ysize = 4 if yev.code == _lib.EKS_YEV32 else 8
    off = (T_ * n * B * ysize + 255) // 256 * 256
    out[key + "_y"] = yev.buf[:T_ * n * B * ysize]
    out[key + "_ev"] = yev.buf[off:off + T_ * n * B * 8]
    out[key + "_code"] = torch.tensor([yev.code])


def run_smooth(torch, d, P, models, algo):
    from eks_amd import batch
    res = batch.smooth(d, device_rows(torch, models), n=P["n"], r=P["r"], want_ms=True,
                       want_nll=True, algo=algo, flags=batch.model_flags(*model_arrays(models)))
    return {k: res[k] for k in ("out", "ms", "nll", "status")}


def run_smooth_var(torch, d, P, models, _):
    from eks_amd import batch
    return batch.smooth_var(d, device_rows(torch, models), n=P["n"], r=P["r"], want_Vs=True)


def run_nll_sweep(torch, d, P, models, _):
    from eks_amd import batch
    K, B = len(SCALES), d.shape[0]
    status = torch.empty((K, B), dtype=torch.int32, device="cuda")
    nll = batch.nll_sweep(d, device_rows(torch, models, SCALES), K=K, n=P["n"], r=P["r"],
                          check=False, status=status)
    return dict(nll=nll, status=status)


def run_smooth_seg(torch, d, P, models, _):
    from eks_amd import batch, timeshard
    res = timeshard.smooth_segments(d, device_rows(torch, models), n=P["n"], r=P["r"], nseg=NSEG,
                                    flags=batch.model_flags(*model_arrays(models)), want_ms=True)
    return {k: res[k] for k in ("out", "ms", "nll", "status")}


def fit_kind(P):
    return ("singleview", 50.0) if P["kind"] == "sv" else ("multicam", 25.0)


def run_fit(torch, d, P, models, _):
    from eks_amd import batch
    import test_gpu_fit_gaps as FG
    kind, q = fit_kind(P)
    params, status, yev = batch.fit(d, kind=kind, n=P["n"], r=P["r"], smooth_param=FG.S,
                                    quantile_keep=q, check=False, keep_yev=True)
    out = dict(params=params, status=status)
    yev_planes(torch, yev, out)
    return out


def run_ensemble(torch, d, P, models, mode):
    import eks_amd.ops  # noqa: F401
    preds, var = torch.ops.eks.ensemble(d, mode)
    return dict(preds=preds, var=var)


def run_smooth_gaps(torch, d, P, models, mode):
    from eks_amd import batch
    return batch.smooth_gaps(d, device_rows(torch, models), n=P["n"], r=P["r"], mode=mode,
                             want_var=True, want_Vs=True, want_ms=True, want_nll=True)


def run_nll_sweep_gaps(torch, d, P, models, mode):
    from eks_amd import batch
    return batch.nll_sweep_gaps(d, device_rows(torch, models, SCALES), K=len(SCALES), n=P["n"],
                                r=P["r"], mode=mode, check=False)


def noise_tensor(torch, z):
    import test_gpu_draws as TD
    return TD.noise_tensor(torch, z)


def run_draws_gaps(torch, d, P, models, mode):
    from eks_amd import batch
    res = batch.draws_gaps(d, device_rows(torch, models), n=P["n"], r=P["r"],
                           noise=noise_tensor(torch, P["z"]), mode=mode, want_latent=True,
                           want_out=True, want_var=True)
    return res


def run_fit_gaps(torch, d, P, models, mode):
    from eks_amd import batch
    import test_gpu_fit_gaps as FG
    kind, q = fit_kind(P)
    res = batch.fit_gaps(d, kind=kind, n=P["n"], r=P["r"], smooth_param=FG.S, quantile_keep=q,
                         mode=mode, check=False)
    out = {k: res[k] for k in ("params", "status", "ncomplete", "nkept")}
    yev_planes(torch, res["yev"], out)
    return out


def run_ensemble_gaps(torch, d, P, models, mode):
    from eks_amd import batch
    res = batch.ensemble_gaps(d, n=P["n"], mode=mode, min_members=2, want_nvalid=True)
    out = dict(nvalid=res["nvalid"])
    yev_planes(torch, res["yev"], out)
    return out


def run_fit_pupil(torch, d, P, models, mode):
    from eks_amd import batch
    res = batch.fit_pupil(d, mode=mode, check=False, keep_yev=True)
    out = {k: res[k] for k in ("stats", "ncomplete", "status")}
    yev_planes(torch, res["yev"], out)
    return out


MODES = ("median", "mean")
# entry -> (runner, the problem's member array, poison, shapes, variants of a shape)
ENTRIES = {
    "smooth": (run_smooth, "st", NAN, tuple(SHAPES), lambda s: (4,) if s == "rt" else (1, 2, 3)),
    "smooth_var": (run_smooth_var, "st", NAN, tuple(SHAPES), lambda s: (None,)),
    "nll_sweep": (run_nll_sweep, "st", NAN, tuple(SHAPES), lambda s: (None,)),
    "smooth_seg": (run_smooth_seg, "st", NAN, COMPILED, lambda s: (None,)),
    "fit": (run_fit, "st", NAN, tuple(SHAPES), lambda s: (None,)),
    "ensemble": (run_ensemble, "st", NAN, tuple(SHAPES), lambda s: MODES),
    "smooth_gaps": (run_smooth_gaps, "g", BIG, tuple(SHAPES), lambda s: MODES),
    "nll_sweep_gaps": (run_nll_sweep_gaps, "g", BIG, tuple(SHAPES), lambda s: MODES),
    "draws_gaps": (run_draws_gaps, "g", BIG, tuple(SHAPES), lambda s: MODES),
    "fit_gaps": (run_fit_gaps, "g", BIG, tuple(SHAPES), lambda s: MODES),
    "ensemble_gaps": (run_ensemble_gaps, "gm", BIG, tuple(SHAPES), lambda s: MODES),
    "fit_pupil": (run_fit_pupil, "pupil", BIG, ("pupil5", "pupil4"), lambda s: MODES),
}


def get_problem(shape, B):
    return pupil_problem(int(shape[5:]), B) if shape.startswith("pupil") else problem(shape, B)


def models_of(P, shared):
    if P["kind"] == "pupil":
        return None
    return shared_models(P["shape"], P["B"]) if shared else P["models"]


_TM = {}


def tm_result(torch, entry, shape, B, dtype, variant):
    """The entry point's outputs on the canonical layout: computed once."""
    key = (entry, shape, B, np.dtype(dtype).name, variant)
    if key not in _TM:
        run, src, poison, _, _ = ENTRIES[entry]
        P = get_problem(shape, B)
        d = LY.make(P[src], "tm", dtype, poison, "cuda")
        _TM[key] = run(torch, d, P, models_of(P, False), variant)
        torch.cuda.synchronize()
    return _TM[key]


# ---------------------------------------------------------------------------
# (b) bit for bit
# ---------------------------------------------------------------------------
def bits(torch, t):
    t = t.contiguous()
    if t.dtype == torch.float64:
        return t.view(torch.int64)
    if t.dtype == torch.float32:
        return t.view(torch.int32)
    return t


def assert_same_bits(torch, got, want, what):
    assert set(got) == set(want), (what, sorted(got), sorted(want))
    for k in sorted(want):
        a, b = got[k], want[k]
        if a is None or b is None:
            assert a is None and b is None, (what, k)
            continue
        assert a.shape == b.shape and a.dtype == b.dtype, (what, k, a.shape, b.shape)
        ia, ib = bits(torch, a), bits(torch, b)
        if not torch.equal(ia, ib):
            nd = int((ia != ib).sum())
            fa, fb = a.contiguous().double(), b.contiguous().double()
            worst = float(torch.nan_to_num((fa - fb).abs(), nan=float("inf")).max()) \
                if a.dtype.is_floating_point else float((ia != ib).sum())
            raise AssertionError(f"{what}: {k} differs in {nd} of {ia.numel()} entries "
                                 f"(max |d| {worst:.3e})")


def assert_aims(built, dtype, B, E, n):
    """The tensor sits on the side of every guard that its layout claims."""
    L, v = built.layout, built.view
    isz = np.dtype(dtype).itemsize
    assert built.base.data_ptr() % 16 == 0, "the allocator's alignment changed"
    assert tuple(v.stride()) == tuple(L.strides(B, T, E, n)), (L.name, v.stride())
    mod = v.data_ptr() % 16
    assert (mod == 0) == L.aligned16, (L.name, mod)
    if not L.aligned16:
        assert mod == L.offset * isz, (L.name, mod)
    assert LY.predicates(v.stride(), mod, isz, B, E, n) == L.claims(isz, B, T, E, n), L.name


def cases(names=LY.NAMES, bs=BS):
    """(layout, dtype, B) of every applicable combination; a shared layout
    needs B > 1 (k_c0_shared; B = 1 with sb = 0 is bm)."""
    out = []
    for name in names:
        if name == "tm":
            continue
        for dtype in DTYPES:
            if not LY.applies(name, dtype):
                continue
            for B in bs:
                if LY.LAYOUTS[name].shared and B == 1:
                    continue
                tag = "f32" if dtype is np.float32 else "f64"
                out.append(pytest.param(name, dtype, B, id=f"{name}-{tag}-B{B}"))
    return out


def check_layout(torch, entry, name, dtype, B):
    run, src, poison, shapes, variants = ENTRIES[entry]
    shared = LY.LAYOUTS[name].shared
    for shape in shapes:
        P = get_problem(shape, B)
        built = LY.build(P[src], name, dtype, poison, "cuda")
        assert_aims(built, dtype, B, P["E"], P["n"])
        models = models_of(P, shared)
        partner = built.view.contiguous() if shared else None
        for variant in variants(shape):
            what = f"{entry} {shape} {variant} {name} {np.dtype(dtype).name} B={B}"
            got = run(torch, built.view, P, models, variant)
            if shared:
                assert partner.stride(0) == T * P["E"] * P["n"] and partner.data_ptr() % 16 == 0
                want = run(torch, partner, P, models, variant)
            else:
                want = tm_result(torch, entry, shape, B, dtype, variant)
            torch.cuda.synchronize()
            assert_same_bits(torch, got, want, what)


@pytest.mark.parametrize("name,dtype,B", cases())
def test_layout_smooth(torch, name, dtype, B):
    check_layout(torch, "smooth", name, dtype, B)


@pytest.mark.parametrize("name,dtype,B", cases())
def test_layout_smooth_var(torch, name, dtype, B):
    check_layout(torch, "smooth_var", name, dtype, B)


@pytest.mark.parametrize("name,dtype,B", cases())
def test_layout_nll_sweep(torch, name, dtype, B):
    check_layout(torch, "nll_sweep", name, dtype, B)


@pytest.mark.parametrize("name,dtype,B", cases())
def test_layout_smooth_seg(torch, name, dtype, B):
    check_layout(torch, "smooth_seg", name, dtype, B)


@pytest.mark.parametrize("name,dtype,B", cases())
def test_layout_fit(torch, name, dtype, B):
    check_layout(torch, "fit", name, dtype, B)


@pytest.mark.parametrize("name,dtype,B", cases())
def test_layout_ensemble(torch, name, dtype, B):
    check_layout(torch, "ensemble", name, dtype, B)


@pytest.mark.parametrize("name,dtype,B", cases())
def test_layout_smooth_gaps(torch, name, dtype, B):
    check_layout(torch, "smooth_gaps", name, dtype, B)


@pytest.mark.parametrize("name,dtype,B", cases())
def test_layout_nll_sweep_gaps(torch, name, dtype, B):
    check_layout(torch, "nll_sweep_gaps", name, dtype, B)


@pytest.mark.parametrize("name,dtype,B", cases())
def test_layout_draws_gaps(torch, name, dtype, B):
    check_layout(torch, "draws_gaps", name, dtype, B)


@pytest.mark.parametrize("name,dtype,B", cases())
def test_layout_fit_gaps(torch, name, dtype, B):
    check_layout(torch, "fit_gaps", name, dtype, B)


@pytest.mark.parametrize("name,dtype,B", cases())
def test_layout_ensemble_gaps(torch, name, dtype, B):
    check_layout(torch, "ensemble_gaps", name, dtype, B)


@pytest.mark.parametrize("name,dtype,B", cases())
def test_layout_fit_pupil(torch, name, dtype, B):
    """B = 1 is where ``packed`` meets ``row1`` (the planes stored by row)."""
    check_layout(torch, "fit_pupil", name, dtype, B)


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_one_element_off_is_seen(torch, entry):
    """The control of (b): the bm tensor read one element further on (inside
    the allocation, by the guard: its last element is then poison) does not
    give the bits of ``tm`` in any entry point, the last variant of each
    (algo 3, "mean") included."""
    run, src, poison, shapes, variants = ENTRIES[entry]
    B, dtype = 3, np.float32
    for shape in shapes:
        P = get_problem(shape, B)
        built = LY.build(P[src], "bm", dtype, poison, "cuda")
        v = built.view
        off = built.base.as_strided(tuple(v.shape), tuple(v.stride()), v.storage_offset() + 1)
        variant = variants(shape)[-1]
        got = run(torch, off, P, models_of(P, False), variant)
        torch.cuda.synchronize()
        with pytest.raises(AssertionError, match="differs"):
            assert_same_bits(torch, got, tm_result(torch, entry, shape, B, dtype, variant),
                             f"{entry} {shape} one element off")


# ---------------------------------------------------------------------------
# (a) the canonical layout against the CPU references
# ---------------------------------------------------------------------------
def test_shapes_span_several_chunks(torch):
    """T = 613 is several chunks in every time-parallel form, at every B."""
    from eks_amd import _lib
    lib = _lib.load()
    K = len(SCALES)
    for B in BS:
        for r in (2, 3):
            for L in (lib.eks_smooth_chunk_len(B, T, r), lib.eks_smooth_var_chunk_len(B, T, r),
                      lib.eks_nll_sweep_chunk_len(B, K, T, r),
                      lib.eks_smooth_gaps_chunk_len(B, T, r),
                      lib.eks_nll_sweep_gaps_chunk_len(B, K, T, r),
                      lib.eks_draws_gaps_chunk_len(B, T, r)):
                assert 0 < L and 3 * L < T, (B, r, L)
        for shape in COMPILED:
            r, n, E = SHAPES[shape]
            for algo in (1, 2, 3):
                assert _lib.plan_info(B, T, n, r, E, algo)["algo"] == algo
        assert _lib.plan_info(B, T, 10, 3, 5, 4)["algo"] == 4
    assert T > 2 * 256 and T % 4 and T % 64 and T % 256


AB = [pytest.param(s, B, dt, id=f"{s}-B{B}-{'f32' if dt is np.float32 else 'f64'}")
      for s in SHAPES for B in BS for dt in DTYPES]
AB_COMPILED = [p for p in AB if p.values[0] in COMPILED]


def np_(t):
    return t.cpu().numpy()


def oracle_models(P, rows):
    ms = []
    for b in rows:
        m = dict(P["models"][b])
        m["offset"] = m["means"]
        ms.append(m)
    return ms


def anchor_smooth(res, P, rows, what):
    """out, ms and nll as test_gpu_parity.py holds them against the oracle."""
    import test_gpu_parity as TP
    from oracle import eks_oracle as O
    ms_ = oracle_models(P, rows)
    ref = TP._oracle_smooth_batch([P["st"][b] for b in rows], ms_, O)
    out, nll = np_(res["out"]), np_(res["nll"])
    assert not np_(res["status"]).any(), what
    err = max(float(np.abs(out[b] - ref[i]).max()) for i, b in enumerate(rows))
    print(f"[layouts] {what}: out {err:.3e} px")
    assert err < TP.OUT_TOL, (what, err)
    for i, b in enumerate(rows):
        m = ms_[i]
        preds, ev = O.ensemble_array(P["st"][b])
        want = O.compute_nll(preds - m["offset"], m["m0"], m["S0"], m["C"], m["A"], m["Q"], ev)
        assert abs(float(nll[b]) - want) <= 1e-9 * abs(want), (what, b)
        if res.get("ms") is not None:
            proj = np_(res["ms"])[b] @ m["C"].T + m["offset"]
            assert float(np.abs(proj - ref[i]).max()) < TP.OUT_TOL, (what, b)


@pytest.mark.parametrize("shape,B,dtype", AB)
def test_tm_smooth(torch, shape, B, dtype):
    P = problem(shape, B)
    for algo in ENTRIES["smooth"][4](shape):
        anchor_smooth(tm_result(torch, "smooth", shape, B, dtype, algo), P, ANCHOR_ROWS(B),
                      f"smooth {shape} B={B} algo={algo}")


@pytest.mark.parametrize("shape,B,dtype", AB_COMPILED)
def test_tm_smooth_seg(torch, shape, B, dtype):
    anchor_smooth(tm_result(torch, "smooth_seg", shape, B, dtype, None), problem(shape, B),
                  ANCHOR_ROWS(B), f"smooth_seg {shape} B={B}")


@pytest.mark.parametrize("shape,B,dtype", AB)
def test_tm_smooth_var(torch, shape, B, dtype):
    import test_gpu_postvar as PV
    P = problem(shape, B)
    res = tm_result(torch, "smooth_var", shape, B, dtype, None)
    rows = ANCHOR_ROWS(B)
    assert not np_(res["status"]).any()
    refs = [PV.oracle_var(P["st"][b], P["models"][b]) for b in rows]
    PV.close(np_(res["var"])[rows], np.stack([v for _, v in refs]), f"var {shape} B={B}")
    PV.close(np_(res["Vs"])[rows], np.stack([V for V, _ in refs]), f"Vs {shape} B={B}")


@pytest.mark.parametrize("shape,B,dtype", AB)
def test_tm_nll_sweep(torch, shape, B, dtype):
    import test_gpu_sweep as TS
    P = problem(shape, B)
    res = tm_result(torch, "nll_sweep", shape, B, dtype, None)
    rows = ANCHOR_ROWS(B)
    assert not np_(res["status"]).any()
    ref = np.array([[SD.oracle_nll(P["st"][b], P["models"][b], s) for b in rows] for s in SCALES])
    TS.close(np_(res["nll"])[:, rows], ref, f"nll_sweep {shape} B={B}", TS.RTOL_ORACLE)


def host_fit_blocks(got, ref, kind, FG):
    """The device fit against the host fit, block by block, with the bounds of
    test_gpu_parity.py / test_gpu_fit_gaps.py."""
    if kind == "singleview":
        for k in ("m0", "S0", "A", "Q", "C", "offset"):
            FG._close(got[k], ref[k], 1e-9)
        return
    FG._close(got["offset"], ref["offset"], 1e-9)
    FG._close(got["A"], ref["A"], 1e-9)
    sgn = np.sign(np.sum(got["C"] * ref["C"], axis=0))
    FG._close(got["C"] * sgn, ref["C"], 1e-7)
    FG._close(got["S0"], ref["S0"], 1e-8)
    FG._close(got["Q"] * np.outer(sgn, sgn), ref["Q"], 1e-7)


@pytest.mark.parametrize("shape,B,dtype", AB)
def test_tm_fit(torch, shape, B, dtype):
    import test_gpu_fit_gaps as FG
    from eks_amd import _lib, fit
    P = problem(shape, B)
    res = tm_result(torch, "fit", shape, B, dtype, None)
    kind, q = fit_kind(P)
    assert not np_(res["status"]).any()
    params = np_(res["params"])
    f = fit.singleview_model if kind == "singleview" else fit.multicam_model
    ydt = np.float32 if int(res["yev_code"]) == _lib.EKS_YEV32 else np.float64
    assert (ydt is np.float32) == (dtype is np.float32 and P["E"] % 2 == 1)
    y = np_(res["yev_y"]).view(ydt).reshape(T, P["n"], B)
    ev = np_(res["yev_ev"]).view(np.float64).reshape(T, P["n"], B)
    for b in ANCHOR_ROWS(B):
        preds, var = G.ensemble(P["st"][b])
        host_fit_blocks(FG._unpack(params[b], P["n"], P["r"]), f(preds, var, FG.S, q), kind, FG)
        # the hand-off planes are the ensemble (test_ensemble_member_counts_vs_oracle's bounds)
        np.testing.assert_allclose(y[:, :, b], preds, rtol=0, atol=1e-12)
        np.testing.assert_allclose(ev[:, :, b], var, rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize("shape,B,dtype", AB)
def test_tm_ensemble(torch, shape, B, dtype):
    """test_ensemble_member_counts_vs_oracle's bounds."""
    from oracle import eks_oracle as O
    P = problem(shape, B)
    for mode in MODES:
        res = tm_result(torch, "ensemble", shape, B, dtype, mode)
        for b in ANCHOR_ROWS(B):
            po, vo = O.ensemble_array(P["st"][b], mode)
            np.testing.assert_allclose(np_(res["preds"][b]), po, rtol=0, atol=1e-12)
            np.testing.assert_allclose(np_(res["var"][b]), vo, rtol=1e-13, atol=1e-13)


@functools.lru_cache(maxsize=None)
def gaps_reference(shape, B, mode):
    P = problem(shape, B)
    refs = {}
    for b in ANCHOR_ROWS(B):
        y, ev = G.ensemble(P["g"][b], mode)
        refs[b] = G.dense(y, ev, P["models"][b])
    return refs


@pytest.mark.parametrize("shape,B,dtype", AB)
def test_tm_smooth_gaps(torch, shape, B, dtype):
    import test_gpu_gaps as TG
    P = problem(shape, B)
    mask = gap_mask(B, P["n"], P["kind"])
    assert mask[0, 200:260].all() and mask[0, 0].all() and mask[0, -1].all()
    for mode in MODES:
        res = tm_result(torch, "smooth_gaps", shape, B, dtype, mode)
        assert not np_(res["status"]).any()
        TG.compare(res, gaps_reference(shape, B, mode), f"{shape} B={B} {mode}",
                   rows=ANCHOR_ROWS(B))


@pytest.mark.parametrize("shape,B,dtype", AB)
def test_tm_nll_sweep_gaps(torch, shape, B, dtype):
    import test_gpu_gaps_sweep as TGS
    P = problem(shape, B)
    rows = ANCHOR_ROWS(B)
    cands = [[GS.scaled(P["models"][b], s) for b in rows] for s in SCALES]
    for mode in MODES:
        res = tm_result(torch, "nll_sweep_gaps", shape, B, dtype, mode)
        assert not np_(res["status"]).any()
        ref, nobs = GS.dense_table(P["g"][rows], cands, mode)
        TGS.close(np_(res["nll"])[:, rows], ref, f"{shape} B={B} {mode} vs dense", TGS.RTOL_REF)
        np.testing.assert_array_equal(np_(res["nobs"])[rows], nobs)
        assert nobs[0] < T * P["n"] - 60 * P["n"]


@pytest.mark.parametrize("shape,B,dtype", AB)
def test_tm_draws_gaps(torch, shape, B, dtype):
    import test_gpu_draws as TD
    import test_gpu_gaps as TG
    P = problem(shape, B)
    rows = ANCHOR_ROWS(B)
    for mode in MODES:
        res = tm_result(torch, "draws_gaps", shape, B, dtype, mode)
        assert not np_(res["status"]).any()
        refs = {}
        for b in rows:
            y, ev = G.ensemble(P["g"][b], mode)
            refs[b] = D.draws(y, ev, P["models"][b], P["z"][b])
        TD.compare(res, refs, f"draws {shape} B={B} {mode}", rows=rows)
        dense = gaps_reference(shape, B, mode)
        out, var = np_(res["out"]), np_(res["var"])
        for b in rows:
            assert float(np.abs(out[b] - dense[b]["out"]).max()) <= TG.OUT_TOL
            np.testing.assert_allclose(var[b], dense[b]["var"], rtol=TG.RTOL, atol=TG.ATOL)


@pytest.mark.parametrize("shape,B,dtype", AB)
def test_tm_fit_gaps(torch, shape, B, dtype):
    """test_gpu_fit_gaps.compare: the host route on preds[ok], ev[ok], every
    trajectory; the counts of complete and kept frames exact."""
    import test_gpu_fit_gaps as FG
    P = problem(shape, B)
    kind, q = fit_kind(P)
    for mode in MODES:
        res = tm_result(torch, "fit_gaps", shape, B, dtype, mode)
        kept = FG.compare(res, P["g"], kind, q, mode, f"{shape} B={B} {mode}", need_finite=True)
        assert min(kept) >= 10, kept
        assert int(res["ncomplete"][0]) < T - 60


@pytest.mark.parametrize("shape,B,dtype", AB)
def test_tm_ensemble_gaps(torch, shape, B, dtype):
    """test_gpu_ensemble_gaps.test_parity's comparison: the counts and the NaN
    patterns exact, the median exact, the mean and the variance to MEAN_TOL /
    EV_RTOL."""
    import test_gpu_ensemble_gaps as EG
    P = problem(shape, B)
    g, n = P["gm"], P["n"]
    xmax = float(np.abs(g[np.isfinite(g)]).max())
    for mode in MODES:
        res = tm_result(torch, "ensemble_gaps", shape, B, dtype, mode)
        assert int(res["yev_code"]) == 3
        y, ev, m = R.ensemble_valid(g.transpose(1, 0, 2, 3), mode, 2)  # (B, T, n)
        yd, ed = (np_(res[k]).view(np.float64).reshape(T, n, B).transpose(2, 0, 1)
                  for k in ("yev_y", "yev_ev"))
        np.testing.assert_array_equal(np_(res["nvalid"]).transpose(2, 0, 1), m)
        assert set(range(P["E"] + 1)) <= set(np.unique(m).tolist())
        np.testing.assert_array_equal(np.isnan(yd), np.isnan(y))
        np.testing.assert_array_equal(np.isnan(ed), np.isnan(ev))
        ok = ~np.isnan(y)
        if mode == "median":
            np.testing.assert_array_equal(yd, y)
        else:
            assert float(np.abs(yd[ok] - y[ok]).max()) <= EG.MEAN_TOL * xmax
        pos = ok & (ev > 0)
        np.testing.assert_array_equal(ed[ok & ~pos], ev[ok & ~pos])
        assert float((np.abs(ed[pos] - ev[pos]) / ev[pos]).max()) <= EG.EV_RTOL


@pytest.mark.parametrize("E", [5, 4])
@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_tm_fit_pupil(torch, E, B, dtype):
    import test_gpu_fit_pupil as FP
    P = pupil_problem(E, B)
    for mode in MODES:
        res = tm_result(torch, "fit_pupil", f"pupil{E}", B, dtype, mode)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            want, cnt = FP.host_stats(P["pupil"], mode)
        assert not np_(res["status"]).any()
        np.testing.assert_array_equal(np_(res["ncomplete"]), cnt)
        assert (cnt < T - 60).all() and (cnt > T // 2).all()
        assert FP.rel_err(np_(res["stats"]), want) <= FP.STAT_RTOL
        # the planes are ensemble_gaps(min_members = E)'s, to its bounds
        y, ev, _ = R.ensemble_valid(P["pupil"].transpose(1, 0, 2, 3), mode, E)
        yd = np_(res["yev_y"]).view(np.float64).reshape(T, 8, B).transpose(2, 0, 1)
        np.testing.assert_array_equal(np.isnan(yd), np.isnan(y))


# ---------------------------------------------------------------------------
# the C++ operators forward the strides
# ---------------------------------------------------------------------------
def op_dict(res, B, n):
    """An operator's result tuple by position; a hand-off buffer (uint8, mean
    mode: EKS_YEV64) as its two planes, without the padding between them."""
    import torch
    out = {}
    for i, t in enumerate(res):
        if t.dtype == torch.uint8:
            sz = T * n * B * 8
            off = (sz + 255) // 256 * 256
            assert t.numel() >= off + sz
            out[f"{i}_y"], out[f"{i}_ev"] = t[:sz], t[off:off + sz]
        else:
            out[i] = t
    return {str(k): v for k, v in out.items()}


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("name", ["bm_off1", "coord_major"])
def test_torch_ops_forward_strides(torch, name, dtype):
    """torch.ops.eks.{smooth, smooth_gaps, fit_gaps, fit_pupil} on a layout
    against the same operator on ``tm``, bit for bit: torch_ops.cpp passes
    obs.stride(0..3) on and does not assume a contiguous tensor."""
    import eks_amd.ops  # noqa: F401
    import test_gpu_fit_gaps as FG
    from eks_amd import batch
    B = 3
    ops = torch.ops.eks
    for shape in ("sv4", "mc"):
        P = problem(shape, B)
        n, r = P["n"], P["r"]
        rows = device_rows(torch, P["models"])
        flags = batch.model_flags(*model_arrays(P["models"]))
        kind, q = fit_kind(P)
        for src, poison, call in (
                ("st", NAN, lambda d: ops.smooth(d, rows, n, r, "median", flags, 0)),
                ("g", BIG, lambda d: ops.smooth_gaps(d, rows, n, r, "mean")),
                ("g", BIG, lambda d: ops.fit_gaps(d, kind, n, r, FG.S, q, "mean"))):
            built = LY.build(P[src], name, dtype, poison, "cuda")
            assert_aims(built, dtype, B, P["E"], n)
            got = call(built.view)
            want = call(LY.make(P[src], "tm", dtype, poison, "cuda"))
            torch.cuda.synchronize()
            assert len(got) == len(want)
            assert_same_bits(torch, op_dict(got, B, n), op_dict(want, B, n),
                             f"op {shape} {src} {name}")
    P = pupil_problem(5, B)
    built = LY.build(P["pupil"], name, dtype, BIG, "cuda")
    assert_aims(built, dtype, B, 5, 8)
    got = ops.fit_pupil(built.view, "mean")
    want = ops.fit_pupil(LY.make(P["pupil"], "tm", dtype, BIG, "cuda"), "mean")
    assert_same_bits(torch, op_dict(got, B, 8), op_dict(want, B, 8), f"op fit_pupil {name}")
    ref = tm_result(torch, "fit_pupil", "pupil5", B, dtype, "mean")
    assert_same_bits(torch, dict(stats=got[0], ncomplete=got[1]),
                     dict(stats=ref["stats"], ncomplete=ref["ncomplete"]), "op vs batch")


@pytest.mark.parametrize("name", ["tm", "coord_major"])
def test_draws_noise_layouts(torch, name):
    """The noise of eks_draws_gaps (i) as a stride(3) == 1 slice of a larger
    buffer, which batch.draws_gaps and the operator pass through as it is, and
    (ii) with stride(3) != 1, which the operator makes contiguous: the draws
    of the default noise tensor, bit for bit."""
    import eks_amd.ops  # noqa: F401
    from eks_amd import batch
    B, shape = 3, "mc"
    P = problem(shape, B)
    n, r = P["n"], P["r"]
    rows = device_rows(torch, P["models"])
    d = LY.make(P["g"], name, np.float32, BIG, "cuda")
    ref = tm_result(torch, "draws_gaps", shape, B, np.float32, "median")
    z = torch.from_numpy(np.array(P["z"])).cuda()  # (B, S, T, r)
    big = torch.full((B, NDRAWS + 1, T + 2, r + 2), BIG, dtype=torch.float64, device="cuda")
    sl = big[:, 1:, 1:T + 1, 1:r + 1]
    sl.copy_(z)
    assert sl.stride(3) == 1 and not sl.is_contiguous() and sl.storage_offset() > 0
    res = batch.draws_gaps(d, rows, n=n, r=r, noise=sl, want_latent=True, want_var=True)
    torch.cuda.synchronize()
    assert_same_bits(torch, {k: res[k] for k in ("draws", "latent", "out", "var", "status")},
                     {k: ref[k] for k in ("draws", "latent", "out", "var", "status")},
                     f"noise slice {name}")
    op_ref = dict(draws=ref["draws"], latent=ref["latent"], out=ref["out"], status=ref["status"])
    got = torch.ops.eks.draws_gaps(d, rows, sl, n, r, "median")
    assert_same_bits(torch, dict(zip(("draws", "latent", "out", "status"), got)), op_ref,
                     f"op noise slice {name}")
    zt = big.new_full((B, NDRAWS, r + 1, T + 1), BIG)[:, :, 1:, 1:].permute(0, 1, 3, 2)
    zt.copy_(z)
    assert zt.stride(3) != 1 and zt.shape == z.shape
    got = torch.ops.eks.draws_gaps(d, rows, zt, n, r, "median")
    assert_same_bits(torch, dict(zip(("draws", "latent", "out", "status"), got)), op_ref,
                     f"op noise transposed {name}")
    with pytest.raises(ValueError):
        batch.draws_gaps(d, rows, n=n, r=r, noise=zt)


# ---------------------------------------------------------------------------
# output strides
# ---------------------------------------------------------------------------
OUT_CASES = [pytest.param(o, B, id=f"{o}-B{B}") for o in LY.OUT_NAMES for B in BS]


def assert_out_aims(view, name, B, n):
    assert tuple(view.stride()) == tuple(LY.OUT_LAYOUTS[name].strides(B, T, n)), name
    lead = B * n + 8 + LY.OUT_LAYOUTS[name].offset  # the guard, then the layout's own offset
    assert view.data_ptr() - view._base.data_ptr() == 8 * lead


@pytest.mark.parametrize("oname,B", OUT_CASES)
def test_out_strides_smooth(torch, oname, B):
    """batch.smooth(out=view), algo 1, 2, 3 (4 on the runtime-n shape): the
    default layout's values bit for bit, nothing outside the view written."""
    from eks_amd import batch
    for shape in ("sv5", "mc", "rt"):
        P = problem(shape, B)
        d = LY.make(P["st"], "tm", np.float32, NAN, "cuda")
        rows = device_rows(torch, P["models"])
        flags = batch.model_flags(*model_arrays(P["models"]))
        for algo in ENTRIES["smooth"][4](shape):
            view, check = LY.make_out(B, T, P["n"], oname, "cuda")
            assert_out_aims(view, oname, B, P["n"])
            res = batch.smooth(d, rows, n=P["n"], r=P["r"], out=view, want_ms=True, want_nll=True,
                               algo=algo, flags=flags)
            torch.cuda.synchronize()
            assert res["out"] is view
            ref = tm_result(torch, "smooth", shape, B, np.float32, algo)
            assert_same_bits(torch, {k: res[k] for k in ("out", "ms", "nll", "status")}, ref,
                             f"smooth out={oname} {shape} B={B} algo={algo}")
            check()


def _mode(mode):
    from eks_amd import _lib
    return _lib.EKS_MEDIAN if mode == "median" else _lib.EKS_MEAN


@pytest.mark.parametrize("oname,B", OUT_CASES)
def test_out_strides_smooth_gaps(torch, oname, B):
    """eks_smooth_gaps through the C ABI: out and pvar (which shares out's
    strides) as views of two canary buffers."""
    from eks_amd import _lib, batch
    lib = _lib.load()
    for shape in ("sv5", "mc", "rt"):
        P = problem(shape, B)
        n, r, E = P["n"], P["r"], P["E"]
        d = LY.make(P["g"], "tm", np.float32, BIG, "cuda")
        rows = device_rows(torch, P["models"])
        out, check_out = LY.make_out(B, T, n, oname, "cuda")
        var, check_var = LY.make_out(B, T, n, oname, "cuda")
        assert_out_aims(out, oname, B, n)
        assert var.stride() == out.stride()
        f64 = dict(dtype=torch.float64, device="cuda")
        Vs, ms, nll = torch.empty((B, T, r, r), **f64), torch.empty((B, T, r), **f64), \
            torch.empty((B,), **f64)
        nobs = torch.empty((B,), dtype=torch.int32, device="cuda")
        status = torch.empty((B,), dtype=torch.int32, device="cuda")
        ws = batch.workspace(lib.eks_smooth_gaps_workspace_bytes(B, T, n, r), "cuda",
                             slot="smooth_gaps")
        sb, st, se, sj = d.stride()
        ob, ot, oj = out.stride()
        _lib.check(lib.eks_smooth_gaps(
            d.data_ptr(), _lib.EKS_F32, B, T, E, n, r, sb, st, se, sj, _mode("mean"),
            rows.data_ptr(), out.data_ptr(), ob, ot, oj, var.data_ptr(), ms.data_ptr(),
            Vs.data_ptr(), nll.data_ptr(), nobs.data_ptr(), ws.data_ptr(), ws.numel(),
            status.data_ptr(), _lib.stream_ptr()), "eks_smooth_gaps")
        torch.cuda.synchronize()
        ref = tm_result(torch, "smooth_gaps", shape, B, np.float32, "mean")
        assert_same_bits(torch, dict(out=out, var=var, Vs=Vs, ms=ms, nll=nll, nobs=nobs,
                                     status=status), ref, f"smooth_gaps out={oname} {shape} B={B}")
        check_out()
        check_var()


@pytest.mark.parametrize("oname,B", OUT_CASES)
def test_out_strides_smooth_var(torch, oname, B):
    from eks_amd import _lib, batch
    lib = _lib.load()
    for shape in ("sv5", "mc", "rt"):
        P = problem(shape, B)
        n, r, E = P["n"], P["r"], P["E"]
        d = LY.make(P["st"], "tm", np.float32, NAN, "cuda")
        rows = device_rows(torch, P["models"])
        var, check = LY.make_out(B, T, n, oname, "cuda")
        assert_out_aims(var, oname, B, n)
        Vs = torch.empty((B, T, r, r), dtype=torch.float64, device="cuda")
        status = torch.empty((B,), dtype=torch.int32, device="cuda")
        ws = batch.workspace(lib.eks_smooth_var_workspace_bytes(B, T, n, r), "cuda",
                             slot="smooth_var")
        sb, st, se, sj = d.stride()
        vb, vt, vj = var.stride()
        _lib.check(lib.eks_smooth_var(
            d.data_ptr(), _lib.EKS_F32, B, T, E, n, r, sb, st, se, sj, rows.data_ptr(),
            var.data_ptr(), vb, vt, vj, Vs.data_ptr(), ws.data_ptr(), ws.numel(),
            status.data_ptr(), _lib.stream_ptr()), "eks_smooth_var")
        torch.cuda.synchronize()
        ref = tm_result(torch, "smooth_var", shape, B, np.float32, None)
        assert_same_bits(torch, dict(var=var, Vs=Vs, status=status), ref,
                         f"smooth_var var={oname} {shape} B={B}")
        check()


@pytest.mark.parametrize("oname,B", OUT_CASES)
def test_out_strides_draws_gaps(torch, oname, B):
    """eks_draws_gaps through the C ABI: the draws (B, S, T, n) as S * B
    (T, n) blocks of an output layout, out and var as in eks_smooth_gaps."""
    from eks_amd import _lib, batch
    lib = _lib.load()
    S = NDRAWS
    for shape in ("sv5", "mc", "rt"):
        P = problem(shape, B)
        n, r, E = P["n"], P["r"], P["E"]
        d = LY.make(P["g"], "tm", np.float32, BIG, "cuda")
        rows = device_rows(torch, P["models"])
        z = noise_tensor(torch, P["z"])
        flat, check_draws = LY.make_out(B * S, T, n, oname, "cuda")
        draws = flat.unflatten(0, (B, S))
        out, check_out = LY.make_out(B, T, n, oname, "cuda")
        var, check_var = LY.make_out(B, T, n, oname, "cuda")
        latent = torch.empty((B, S, T, r), dtype=torch.float64, device="cuda")
        status = torch.empty((B,), dtype=torch.int32, device="cuda")
        ws = batch.workspace(lib.eks_draws_gaps_workspace_bytes(B, S, T, n, r), "cuda",
                             slot="draws_gaps")
        sb, st, se, sj = d.stride()
        zb, zs, zt, z3 = z.stride()
        assert z3 == 1
        db, ds, dtt, dj = draws.stride()
        assert (db, ds) == (S * flat.stride(0), flat.stride(0))
        ob, ot, oj = out.stride()
        _lib.check(lib.eks_draws_gaps(
            d.data_ptr(), _lib.EKS_F32, B, T, E, n, r, sb, st, se, sj, _mode("mean"),
            rows.data_ptr(), S, z.data_ptr(), zb, zs, zt, 0, draws.data_ptr(), db, ds, dtt, dj,
            latent.data_ptr(), out.data_ptr(), ob, ot, oj, var.data_ptr(), ws.data_ptr(),
            ws.numel(), status.data_ptr(), _lib.stream_ptr()), "eks_draws_gaps")
        torch.cuda.synchronize()
        ref = tm_result(torch, "draws_gaps", shape, B, np.float32, "mean")
        assert_same_bits(torch, dict(draws=draws, latent=latent, out=out, var=var, status=status),
                         ref, f"draws_gaps out={oname} {shape} B={B}")
        check_draws()
        check_out()
        check_var()
