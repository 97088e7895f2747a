"""Exact observations (ev == 0: all members agree) off chunk 0 in the
time-parallel smoothers: algo 2 (smooth_impl.hpp), algo 3 (two_pass.hpp) and
algo 4's chunked form (eks_shape_rt.hip) against the sequential algo 1 and
the float64 oracle.

tests/test_gpu_ragged.py covers every shape and kernel form with ev > 0
everywhere; the older exact-agreement tests put ev = 0 at t = 0, inside
chunk 0, where the plain filter runs.  Here the exact entries sit where a
filtering element (kf_steps.hpp Elem, absorb_scalar, elem_absorb) has to
absorb rv = 0: at the first / last step of a chunk >= 1, around a checkpoint
and a unit boundary, in the ragged tail, r columns at once (Ab becomes 0),
over whole chunks and in every frame.  tests/exact_data.py builds the
patterns from the built library's own plan (eks_smooth_plan_info), and
tests/test_exact_host.py shows the oracle is good to ~1e-10 px there.

Rows reuse FORMS and SOURCES of test_gpu_ragged.py and its helpers; as there,
no time-parallel call gets ``check=True`` (it would re-run algo 1 on
EKS_STATUS_SCAN and hide a broken scan) except where the re-run is the
subject (the singular-Q test at the end).
"""
import numpy as np
import pytest

from tests import exact_data as X
from tests.test_gpu_configs import NLL_RTOL, PX_ALGO
from tests.test_gpu_parity import OUT_TOL
from tests.test_gpu_ragged import (FORMS, NLL_ORACLE_RTOL, SOURCES, _assert_form, _compare,
                                   _members, _oracle, _pack, _run, _sample)

SHAPES = [(2, 2), (3, 4), (3, 8), (3, 16)]
FORM_NAMES = ("serial", "group_jd", "uniform", "wave")
EVERY_FORM = ("cycle", "full_rank", "last")
ROTATED = tuple(p for p in X.PATTERNS if p not in EVERY_FORM)
MAX_ORACLE = 12
# one row per shape is fitted with this smoothing parameter instead of 0.05
SMALL_S, SMALL_S_ROW = 0.001, ("serial", "cycle")


def _source(si, fi):
    return SOURCES[(si + fi) % 3]


def _cases():
    rows = []
    for si, (r, n) in enumerate(SHAPES):
        for fi, form in enumerate(FORM_NAMES):
            E, dtype = _source(si, fi)
            B, T, _ = FORMS[form]
            for p in EVERY_FORM:
                rows.append((r, n, E, dtype, B, T, form, p))
        for j, p in enumerate(ROTATED):
            fi = (si + j) % len(FORM_NAMES)
            while p == "ulp" and _source(si, fi)[1] != "f32":   # ulp: float32 members only
                fi = (fi + 1) % len(FORM_NAMES)
            E, dtype = _source(si, fi)
            B, T, _ = FORMS[FORM_NAMES[fi]]
            rows.append((r, n, E, dtype, B, T, FORM_NAMES[fi], p))
    # rows of one (shape, form) cell together: they share members and fits
    return sorted(rows, key=lambda c: (SHAPES.index(c[:2]), FORM_NAMES.index(c[6])))


# (r, n, E, dtype, B, T, form, pattern)
CASES = _cases()
IDS = [f"{r}x{n}-{form}-{p}-B{B}-T{T}-E{E}{dtype}" for r, n, E, dtype, B, T, form, p in CASES]


def test_cases_cover_patterns_forms_and_sources():
    """No GPU: every pattern at every shape, every form sees cycle, full_rank
    and last, the rest rotate over the forms, E = 3, 4 and 5 all appear, every
    row keeps its form and its raggedness (_assert_form, the built library's
    plan) and every pattern can be built on its grid."""
    for r, n, E, dtype, B, T, form, p in CASES:
        _assert_form(r, n, E, B, T, form)
        assert B <= 260 and T <= 421
        X.pattern_jobs(p, X.plan_grid(B, T, n, r, E), r, tuple(range(n)))
        assert p != "ulp" or dtype == "f32"
    for shape in SHAPES:
        rows = [c for c in CASES if c[:2] == shape]
        assert {c[7] for c in rows} == set(X.PATTERNS), shape
        for form in FORM_NAMES:
            assert set(EVERY_FORM) <= {c[7] for c in rows if c[6] == form}, (shape, form)
        assert sum((c[6], c[7]) == SMALL_S_ROW for c in rows) == 1, shape
    # the rotation: over the four shapes a rotated pattern meets every form
    # (ulp: every form whose members are float32 at some shape it is moved to)
    for p in ROTATED:
        forms = {c[6] for c in CASES if c[7] == p}
        assert forms == set(FORM_NAMES) or (p == "ulp" and len(forms) >= 2), (p, forms)
    for shape in SHAPES:
        for form in FORM_NAMES:
            assert any(c[7] in ROTATED for c in CASES if c[:2] == shape and c[6] == form), \
                (shape, form)
    assert {c[2] for c in CASES} == {3, 4, 5}
    assert {(c[2], c[3]) for c in CASES} == set(SOURCES)
    assert len(set(CASES)) == len(CASES)


# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


_cell = {}


def _base(key, r, n, E, dtype, B, T, seed):
    """Members and fitted models of one (shape, form) cell, computed once and
    left unchanged: a pattern refits only the trajectories it changes."""
    if _cell.get("key") != key:
        stacks = _members(np.random.default_rng(seed), r, n, E, dtype, B, T)
        _cell.clear()
        _cell.update(key=key, stacks=stacks, models=X.fit_models(stacks, n))
    return _cell["stacks"], _cell["models"]


def _with_pattern(pattern, stacks, models, grid, r, n, smooth_param=0.05, **kw):
    """The pattern on the cell's members, and the models refitted where it
    changed them (everywhere for another smoothing parameter)."""
    st, mask, changed = X.build(pattern, stacks, grid, r, models=models, **kw)
    if smooth_param != 0.05:
        ms = X.fit_models(st, n, smooth_param)
    else:
        ms = list(models)
        for b, m in zip(changed, X.fit_models(st[changed], n)):
            ms[b] = m
    X.check_conditioning(mask, ms, r)
    return st, mask, changed, ms


def _oracle_rows(B, changed):
    """_sample(B) plus the changed trajectories, at most MAX_ORACLE."""
    rows = _sample(B)
    for b in changed:
        if len(rows) >= MAX_ORACLE:
            break
        if b not in rows:
            rows.append(b)
    assert any(b in rows for b in changed)
    return sorted(rows)


@pytest.mark.gpu
@pytest.mark.parametrize("r,n,E,dtype,B,T,form,pattern", CASES, ids=IDS)
def test_exact_patterns(torch, r, n, E, dtype, B, T, form, pattern):
    """One row: algos 1, 2 and 3 with status == 0 on every trajectory, 2 and 3
    against algo 1 on all of them (PX_ALGO, NLL_RTOL), all three against the
    oracle (OUT_TOL, INT_RTOL, NLL_ORACLE_RTOL) on the sample and the changed
    trajectories; whole trajectory, head and tail."""
    from eks_amd import _lib, batch
    plan = _assert_form(r, n, E, B, T, form)
    grid = X.plan_grid(B, T, n, r, E)
    assert grid["L"] == plan["L"]
    cell = (r, n, form)
    stacks, models = _base(cell, r, n, E, dtype, B, T, 8000 + 10 * SHAPES.index((r, n))
                           + FORM_NAMES.index(form))
    s = SMALL_S if (form, pattern) == SMALL_S_ROW else 0.05
    st, mask, changed, models = _with_pattern(pattern, stacks, models, grid, r, n, s)
    params, flags = _pack(models)
    d = batch.make_time_major(st, dtype=np.float32 if dtype == "f32" else np.float64)
    sample = _oracle_rows(B, changed)
    want = {b: _oracle(st[b], models[b]) for b in sample}
    lib = _lib.load()
    res = {}
    for a in (1, 2, 3):
        assert lib.eks_smooth_algo(B, T, n, r, E, a) == a
        res[a] = _run(batch, d, params, n, r, a, flags)
    worst = {}
    for a in (1, 2, 3):
        worst[a] = _compare(res[a], res[1] if a != 1 else None, want, sample, T, plan["L"],
                            f"{r}x{n} {form} {pattern} B={B} T={T} algo {a}")
    print(f"EXACT pattern={pattern} form={form} shape={r}x{n} B={B} T={T} "
          + " ".join(f"a{a}:d_algo1={worst[a][0]:.3e},d_oracle={worst[a][1]:.3e}" for a in worst))
    if pattern == "agree" and (r, n) == (2, 2):
        # both coordinates observed exactly in every frame: the smoothed output
        # is the observation itself (to the rounding of C ms + offset)
        for a in (1, 2, 3):
            for b in changed:
                assert np.abs(res[a]["out"][b] - st[b, 0]).max() < PX_ALGO, (a, b)


# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("B", [5, 70])
def test_exact_patterns_pupil(torch, B):
    """EKS_MODEL_PUPIL at (3, 8): one exact column per frame (never both of a
    folded pair, so merge_obs sees r1 = 0 or r2 = 0 but not both).  The sparse
    kernels against the dense ones as tests/test_gpu_pupil.py (PX), both
    against the oracle's dense per-step solve on every changed trajectory."""
    from eks_amd import _lib, batch, synthetic
    from oracle import eks_oracle as O
    from tests.test_gpu_pupil import NLL_RTOL as PUPIL_NLL_RTOL
    from tests.test_gpu_pupil import PX, _models
    from tests.test_gpu_pupil import _pack as pupil_pack
    E, T = 5, 421
    rng = np.random.default_rng(600 + B)
    base = np.stack([synthetic.pupil_obs(rng, E, T, a=0.99) for _ in range(B)])
    base = base.astype(np.float32).astype(np.float64)
    diag = [[0.999, 0.99, 0.99], [0.99, 0.999, 0.999], [0.9999, 0.95, 0.95], [0.9, 0.9, 0.9]]
    a_list = [diag[b % 4] for b in range(B)]
    grid = X.plan_grid(B, T, 8, 3, E)
    lib = _lib.load()
    for pattern in ("cycle", "last", "first"):
        st, mask, changed = X.build(pattern, base, grid, 3, pupil=True)
        models = _models([O.ensemble_array(st[b])[0] for b in range(B)], a_list)
        params, flags = pupil_pack(models)
        assert flags == _lib.EKS_MODEL_PUPIL
        d = batch.make_time_major(st, dtype=np.float32)
        rows = _oracle_rows(B, changed)
        want = {b: O.pupil_smooth(st[b], models[b]["A"])[0] for b in rows}
        for algo in (1, 2, 3):
            assert lib.eks_smooth_algo(B, T, 8, 3, E, algo) == algo
            got = {}
            for name, fl in (("dense", 0), ("sparse", flags)):
                res = batch.smooth(d, params, n=8, r=3, algo=algo, flags=fl, want_nll=True,
                                   want_ms=True, check=False)
                status = res["status"].cpu().numpy()
                assert (status == 0).all(), (pattern, algo, name, np.nonzero(status)[0][:8])
                got[name] = {k: res[k].cpu().numpy() for k in ("out", "ms", "nll")}
            what = f"pupil {pattern} B={B} algo {algo}"
            for k in ("out", "ms"):
                dd = float(np.abs(got["sparse"][k] - got["dense"][k]).max())
                assert dd < PX, f"{what}: sparse {k} differs from dense by {dd:.3e}"
            np.testing.assert_allclose(got["sparse"]["nll"], got["dense"]["nll"],
                                       rtol=PUPIL_NLL_RTOL, err_msg=what)
            for name in ("dense", "sparse"):
                for b in rows:
                    dd = float(np.abs(got[name]["out"][b] - want[b]).max())
                    assert dd < OUT_TOL, f"{what}: {name} out[{b}] differs from the oracle by {dd:.3e}"


# ---------------------------------------------------------------------------
@pytest.fixture
def rt_form():
    """eks_debug_set(EKS_DBG_RT_FORM, v) for one test, reset afterwards (the
    fixture of tests/test_gpu_rt.py)."""
    from eks_amd import _lib
    yield lambda v: _lib.debug_set(_lib.EKS_DBG_RT_FORM, v)
    _lib.debug_set(_lib.EKS_DBG_RT_FORM, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("chunked", [0, 2], ids=["auto", "forced"])
@pytest.mark.parametrize("B", [3, 17])
def test_exact_patterns_runtime_n(torch, rt_form, B, chunked):
    """algo 4 at (3, 10): the chunked runtime-n form (chosen by the library,
    EKS_DBG_RT_FORM 0, and forced, 2) against its one-lane form (1) and the
    oracle.  eks_shape_rt.hip cuts the chunks with chunk_len_smooth(B, T, r),
    which does not depend on n: the plan of a compiled r = 3 shape with the
    same (B, T) gives L, and says that the library's own choice is chunked."""
    from eks_amd import _lib, batch
    r, n, T = 3, 10, 421
    E, dtype = SOURCES[B % 3]
    grid = X.plan_grid(B, T, 8, r, E, algo3=False)
    assert -(-T // grid["L"]) > 1 and T % grid["L"] != 0
    assert _lib.load().eks_smooth_algo(B, T, n, r, E, 0) == 4
    stacks = _members(np.random.default_rng(1200 + B), r, n, E, dtype, B, T)
    models = X.fit_models(stacks, n)
    for pattern in ("cycle", "full_rank", "last"):
        st, mask, changed, ms = _with_pattern(pattern, stacks, models, grid, r, n)
        params, flags = _pack(ms)
        d = batch.make_time_major(st, dtype=np.float32 if dtype == "f32" else np.float64)
        sample = _oracle_rows(B, changed)
        want = {b: _oracle(st[b], ms[b]) for b in sample}
        rt_form(1)
        lane = _run(batch, d, params, n, r, 4, flags)
        rt_form(chunked)
        got = _run(batch, d, params, n, r, 4, flags)
        what = f"3x10 rt form {chunked} {pattern} B={B}"
        w1 = _compare(lane, None, want, sample, T, grid["L"], what + " (one lane)")
        w2 = _compare(got, lane, want, sample, T, grid["L"], what)
        print(f"EXACT-RT pattern={pattern} form={chunked} B={B} T={T} lane:d_oracle={w1[1]:.3e} "
              f"chunked:d_lane={w2[0]:.3e},d_oracle={w2[1]:.3e}")


# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("r,n", [(2, 2), (3, 8)])
def test_exact_patterns_filter_only(torch, r, n):
    """Filter-only calls (batch.nll) of algo 2, as test_filter_only_ragged: the
    closed-form NLL share of every chunk (elem_nll_share: log det(I + P Jb)
    with Ab = 0 and a large Jb) under exact observations, on the filter-only
    call's own chunk grid."""
    from eks_amd import batch
    from oracle import eks_oracle as O
    T = 421
    for i, B in enumerate((5, 70)):
        E, dtype = SOURCES[(n // 4 + i) % 3]
        grid = X.plan_grid(B, T, n, r, E, smoothing=False, algo3=False)
        assert T % grid["L"] != 0
        stacks = _members(np.random.default_rng(1500 + 10 * n + i), r, n, E, dtype, B, T)
        models = X.fit_models(stacks, n)
        for pattern in ("cycle", "full_rank"):
            st, mask, changed, ms = _with_pattern(pattern, stacks, models, grid, r, n)
            params, flags = _pack(ms)
            d = batch.make_time_major(st, dtype=np.float32 if dtype == "f32" else np.float64)
            got = {}
            for a in (1, 2):
                status = torch.full((B,), -1, dtype=torch.int32, device="cuda")
                got[a] = batch.nll(d, params, n=n, r=r, algo=a, flags=flags, check=False,
                                   status=status).cpu().numpy()
                assert (status.cpu().numpy() == 0).all(), (B, pattern, a)
            rel = float(np.abs((got[2] - got[1]) / got[1]).max())
            assert rel < NLL_RTOL, (B, pattern, rel)
            worst = 0.0
            for b in _oracle_rows(B, changed):
                m = ms[b]
                preds, ev = O.ensemble_array(st[b])
                ref = O.compute_nll(preds - m["offset"], m["m0"], m["S0"], m["C"], m["A"], m["Q"], ev)
                for a in (1, 2):
                    worst = max(worst, abs(got[a][b] - ref) / abs(ref))
                    assert abs(got[a][b] - ref) <= NLL_ORACLE_RTOL * abs(ref), \
                        (B, pattern, b, a, got[a][b], ref)
            print(f"EXACT-NLL pattern={pattern} shape={r}x{n} B={B} a2 vs a1 rel={rel:.3e} "
                  f"vs oracle rel={worst:.3e}")


# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("algo", [2, 3])
@pytest.mark.parametrize("B", [5, 70])
def test_singular_q_exact_observation_raises_scan(torch, B, algo):
    """EKS_STATUS_SCAN produced the documented way (include/eks_hip.h):
    singular Q with an exact observation.  The scan breaks down only where an
    element starts on the exact frame (tests/test_exact_host.py pins this on
    the numpy model): trajectory 1 (exact at the first step tM of a chunk >= 1
    of the algorithm's own grid) is flagged, trajectory 2 (tM + 1) and
    trajectory 3 (inside chunk 0) are not.  check=True re-runs algo 1."""
    from eks_amd import _lib, batch
    from oracle import eks_oracle as O
    r = n = 2
    E, T = 5, 421
    grid = X.plan_grid(B, T, n, r, E)
    step = grid["L"] if algo == 2 else grid["F"]
    tM = X.mid(step, T)
    assert tM % step == 0 and tM >= step and tM + 1 < T and step >= 4
    st = _members(np.random.default_rng(1700 + B), r, n, E, "f32", B, T)
    for b, t in ((1, tM), (2, tM + 1), (3, step // 2)):
        st[b, :, t, 1] = st[b, 0, t, 1]
    models = []
    for b in range(B):
        preds, ev = O.ensemble_array(st[b])
        assert int((ev == 0).sum()) == (1 if b in (1, 2, 3) else 0)
        models.append(X.singular_q_model(preds))
    params, _ = _pack(models)
    d = batch.make_time_major(st, dtype=np.float32)
    assert _lib.load().eks_smooth_algo(B, T, n, r, E, algo) == algo
    rows = sorted(set(_sample(B)) | {1, 2, 3})
    want = {b: _oracle(st[b], models[b]) for b in rows}

    res = batch.smooth(d, params, n=n, r=r, algo=algo, flags=0, want_nll=True, check=False)
    status = res["status"].cpu().numpy()
    expect = np.zeros(B, dtype=status.dtype)
    expect[1] = _lib.EKS_STATUS_SCAN
    assert status.tolist() == expect.tolist(), (np.nonzero(status != expect)[0], status[:8])
    out = res["out"].cpu().numpy()
    for b in rows:
        if b != 1:
            dd = float(np.abs(out[b] - want[b][0]).max())
            assert dd < OUT_TOL, f"algo {algo} B={B}: out[{b}] differs from the oracle by {dd:.3e}"

    res = batch.smooth(d, params, n=n, r=r, algo=algo, flags=0, want_nll=True, check=True)
    assert (res["status"].cpu().numpy() == 0).all()
    out, nll = res["out"].cpu().numpy(), res["nll"].cpu().numpy()
    for b in rows:
        dd = float(np.abs(out[b] - want[b][0]).max())
        assert dd < OUT_TOL, f"algo {algo} B={B} check=True: out[{b}] off by {dd:.3e}"
        assert abs(nll[b] - want[b][2]) <= NLL_ORACLE_RTOL * abs(want[b][2]), (b, nll[b], want[b][2])
    seq = batch.smooth(d, params, n=n, r=r, algo=1, flags=0, check=False)
    assert (seq["status"].cpu().numpy() == 0).all()
