"""The reference under exact observations (no GPU): the float64 oracle that
tests/test_gpu_exact.py compares the kernels with, against the same
recursions in np.longdouble, on every pattern of tests/exact_data.py at
(2, 2), (3, 4) and (3, 8), T = 101 with 16-step chunks.

The oracle must stay within OUT_TOL / 100 (outputs) and NLL_ORACLE_RTOL / 100
(NLL, relative) of long double, so that its own error takes no part in the
GPU comparison.  Worst values measured over all patterns, shapes and changed
trajectories (printed by the test, -s):

    float64 oracle vs long double, outputs   2.0e-12 px  (run, 3x8; bound 1e-7)
    float64 oracle NLL, relative             5.8e-13     (run, 3x8; bound 1e-11)
    element model's chunk-end states         2.8e-14
    singular-Q model, outputs                2.8e-14 px

run (r columns in every frame of two chunks) is the worst pattern; every
other one stays below 1.4e-12 px and 4.2e-15 relative NLL.  These figures
hold for r exact columns whose rows of C are well conditioned
(exact_data.best_columns / check_conditioning): with the first three columns
(cond up to 88 at 3x8) agree reached 2.0e-10 px and run 2.1e-12 of the NLL
at T = 101, and one T = 421 trajectory 2e-8 px and 1e-8 of the NLL -- the
singular S of more than r exact columns in the limit, an input without a
reference.

Also here: the builders' invariants (at most r exact columns in a frame, no
folded pupil pair, ev == 0 exactly on the mask and nowhere else), and the
numpy element model pinning where a singular Q breaks the scan: only in the
element whose first step is the exact frame.
"""
import numpy as np
import pytest

from tests import exact_data as X
from tests.test_gpu_parity import OUT_TOL
from tests.test_gpu_ragged import NLL_ORACLE_RTOL, SOURCES, _members, _oracle

SHAPES = [(2, 2), (3, 4), (3, 8)]
T, L_HOST, B = 101, 16, 5


def _grid(r, n, E):
    """LS, the fine chunk and the units as the library plans them for this
    shape (at the GPU rows' T); T = 101 and L = 16 as the module docstring."""
    g = X.plan_grid(5, 421, n, r, E)
    g.update(T=T, L=L_HOST)
    assert L_HOST % g["LS"] == 0
    return g


def _source(si, pattern):
    E, dtype = SOURCES[(si + X.PATTERNS.index(pattern)) % 3]
    return (5, "f32") if pattern == "ulp" and dtype != "f32" else (E, dtype)


def _case(si, r, n, pattern, smooth_param=0.05):
    E, dtype = _source(si, pattern)
    rng = np.random.default_rng(4100 + 100 * si + X.PATTERNS.index(pattern))
    base = _members(rng, r, n, E, dtype, B, T)
    st, mask, changed = X.build(pattern, base, _grid(r, n, E), r, models=X.fit_models(base, n))
    return st, mask, changed


@pytest.mark.parametrize("pattern", X.PATTERNS)
@pytest.mark.parametrize("si", range(len(SHAPES)), ids=[f"{r}x{n}" for r, n in SHAPES])
def test_oracle_within_margin_of_long_double(si, pattern):
    from oracle import eks_oracle as O
    r, n = SHAPES[si]
    st, mask, changed = _case(si, r, n, pattern)
    assert changed
    for b in changed:
        _, ev = O.ensemble_array(st[b])
        if pattern == "ulp":
            assert ((ev[mask[b]] > 0) & (ev[mask[b]] < 1e-9)).all() and (ev > 0).all()
        else:
            assert np.array_equal(ev == 0, mask[b]), "ev == 0 exactly on the mask, > 0 elsewhere"
    for b in sorted(X.clean_rows(B)):
        assert (O.ensemble_array(st[b])[1] > 0).all()
    # 0.001 for the cycle row of every shape, 0.05 (as _fit_models) elsewhere
    models = X.fit_models(st, n, 0.001 if pattern == "cycle" else 0.05)
    X.check_conditioning(mask, models, r)
    d_out = d_nll = 0.0
    for b in changed:
        out, _, nll = _oracle(st[b], models[b])           # raises LinAlgError if singular
        out_ld, nll_ld, _, _ = X.reference(st[b], models[b], np.longdouble)
        d_out = max(d_out, float(np.abs(out - out_ld).max()))
        d_nll = max(d_nll, abs(float((nll - nll_ld) / nll_ld)))
        if pattern == "agree" and (r, n) == (2, 2):   # both coordinates observed exactly
            assert np.abs(out - st[b, 0]).max() < 1e-9
    print(f"EXACT-HOST pattern={pattern} shape={r}x{n} out64-ld={d_out:.2e} nll rel={d_nll:.2e}")
    assert d_out < OUT_TOL / 100, d_out
    assert d_nll < NLL_ORACLE_RTOL / 100, d_nll


def test_pupil_patterns_keep_the_pair_rule():
    from eks_amd import synthetic
    from oracle import eks_oracle as O
    rng = np.random.default_rng(5)
    st = np.stack([synthetic.pupil_obs(rng, 5, T, a=0.99) for _ in range(B)])
    st = st.astype(np.float32).astype(np.float64)
    for pattern in ("cycle", "last", "first"):
        ex, mask, changed = X.build(pattern, st, _grid(3, 8, 5), 3, pupil=True)
        X.check_invariants(mask, 3, pupil=True)
        folded = {c for pair in X.PUPIL_PAIRS for c in pair}
        assert folded & set(np.nonzero(mask.any(axis=(0, 1)))[0]), pattern  # merge_obs sees rv = 0
        for b in changed:
            assert np.array_equal(O.ensemble_array(ex[b])[1] == 0, mask[b])
    bad = np.zeros((B, T, 8), dtype=bool)
    bad[1, 7, [5, 7]] = True
    with pytest.raises(AssertionError):
        X.check_invariants(bad, 3, pupil=True)
    bad = np.zeros((B, T, 8), dtype=bool)
    bad[1, 7, :4] = True
    with pytest.raises(AssertionError):
        X.check_invariants(bad, 3)
    # nearly dependent rows of C in one frame: the singular S in the limit
    bad = np.zeros((B, T, 8), dtype=bool)
    bad[1, 7, :3] = True
    C = np.eye(8, 3)
    C[2] = C[0] + 1e-3 * C[2]
    with pytest.raises(AssertionError):
        X.check_conditioning(bad, [dict(C=C)] * B, 3)
    assert X.best_columns(np.vstack([C, np.eye(3)[2:]]), 3) in ((0, 1, 8), (1, 2, 8))


def test_element_model_matches_the_filter():
    """compose_state of the numpy element model reproduces the long-double
    filtered state at every chunk end, exact observations included: the
    algorithm itself allows them (the model is the yardstick of the
    singular-Q claim below, so it is checked first)."""
    from oracle import eks_oracle as O
    worst = 0.0
    for si, (r, n) in enumerate(SHAPES):
        for pattern in ("full_rank", "cycle", "run"):
            st, mask, changed = _case(si, r, n, pattern)
            models = X.fit_models(st[changed], n)
            for b, m in zip(changed, models):
                preds, ev = O.ensemble_array(st[b])
                y = preds - m["offset"]
                _, _, mf, Vf = X.reference(st[b], m, np.longdouble)
                mm, P = np.asarray(mf[L_HOST - 1], float), np.asarray(Vf[L_HOST - 1], float)
                for s in range(L_HOST, T, L_HOST):
                    e = min(s + L_HOST, T)
                    el = X.elem(y, ev, m, s, e)
                    assert el[5], (r, n, pattern, b, s)
                    mm, P = X.compose_state(mm, P, el)
                    worst = max(worst, float(np.abs(mm - np.asarray(mf[e - 1], float)).max()),
                                float(np.abs(P - np.asarray(Vf[e - 1], float)).max()))
    print(f"EXACT-HOST element model vs long double, chunk-end states: {worst:.2e}")
    assert worst < OUT_TOL / 100, worst


def test_singular_q_breaks_only_the_element_that_starts_on_the_exact_frame():
    """EKS_STATUS_SCAN's documented cause: Q singular and an exact observation
    in its null direction at the first step of a chunk >= 1.  The element of
    the chunk [kL, (k+1)L) reports a non-positive pivot if and only if the
    exact frame is kL; the reference is regular wherever the frame is."""
    from eks_amd import _lib
    from oracle import eks_oracle as O
    Tq = 421
    L = _lib.plan_info(5, Tq, 2, 2, 5, 2)["L"]
    assert 2 <= L and 3 * L < Tq
    rng = np.random.default_rng(3)
    base = _members(rng, 2, 2, 5, "f32", 1, Tq)[0]
    for tex in (L, L + 1, L + 2, 2 * L - 1, L // 2):
        st = base.copy()
        st[:, tex, 1] = st[0, tex, 1]
        preds, ev = O.ensemble_array(st)
        assert ev[tex, 1] == 0 and int((ev == 0).sum()) == 1
        m = X.singular_q_model(preds)
        y = preds - m["offset"]
        for k in range(1, 4):
            ok = X.elem(y, ev, m, k * L, (k + 1) * L)[5]
            assert ok == (tex != k * L), (tex, k, ok)
        out, _, _ = _oracle(st, m)
        out_ld = X.reference(st, m, np.longdouble)[0]
        d = float(np.abs(out - out_ld).max())
        print(f"EXACT-HOST singular Q, exact column 1 at t={tex}: out64-ld={d:.2e}")
        assert d < OUT_TOL / 100, (tex, d)
