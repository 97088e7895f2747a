"""The time-parallel smoothers (algo 2: smooth_impl.hpp, algo 3: two_pass.hpp)
off every chunk grid, in every kernel form the host picks from (B, T).

One table, CASES, drives everything.  Each row names the form it must take
(serial chunk scans, group mode, group mode with (J, d) planes, uniform lanes,
wave-parallel scans without groups); ``test_cases_stay_on_the_edges`` asks the
built library (eks_smooth_plan_info, host only) whether the row still takes
that form and whether T is still ragged on every grid: the last chunk (L), the
last checkpoint sub-chunk (LS), algo 3's last fine chunk and its last unit.
When a retuning of chunk_len / kMinChunk / wave_scan_chunks / fine_len3 moves
a row off its edge, that test fails and the row's (B, T) has to move with it.

The GPU tests never pass ``check=True`` to a time-parallel call (it would
re-run algo 1 on EKS_STATUS_SCAN and hide a broken scan): they assert
status == 0 themselves, compare algos 2 and 3 with the sequential algo 1 on
every trajectory and all three with the float64 oracle on a fixed sample of
trajectories, and repeat both comparisons on the first L and the last 2 L
frames so that a tail defect is reported as one.

Chained scans of more than one block per trajectory (G > 1) need T above
~170 000 in group mode at r = 3: tests/test_gpu_chain.py and the full-size
configuration tests cover them, this file asserts G == 1.
"""
import itertools

import numpy as np
import pytest

from tests.test_gpu_configs import NLL_RTOL, PX_ALGO
from tests.test_gpu_parity import INT_RTOL, OUT_TOL, _close

NLL_ORACLE_RTOL = 1e-9   # NLL against oracle.compute_nll (as test_fused_batch_vs_oracle)

SHAPES = [(2, 2), (3, 4), (3, 6), (3, 8), (3, 12), (3, 16)]
# member sources: float32 with an odd-E median (y is stored as float), float32
# with an even E (y stored as double), float64
SOURCES = [(5, "f32"), (4, "f32"), (3, "f64")]
# form -> (B, T, what eks_smooth_plan_info must say of a smoothing algo-2 call)
FORMS = {
    "serial": (5, 131, dict(uniform_lanes=0, wave_scan=0, grp=0, jd=0)),
    "group": (3, 421, dict(uniform_lanes=0, wave_scan=1, grp=1, jd=0)),
    # (2, 2) has no (J, d) kernels: there this is plain group mode with B >= 8
    "group_jd": (70, 421, dict(uniform_lanes=0, wave_scan=1, grp=1, jd=1)),
    "uniform": (230, 421, dict(uniform_lanes=1, wave_scan=1, grp=0, jd=0)),
    "wave": (260, 421, dict(uniform_lanes=0, wave_scan=1, grp=0, jd=0)),
}
# T = 421 is ragged on every grid at once (421 % 2, 4, 8, 16, 5, 7 = 1, 1, 5, 5,
# 1, 1; 27 chunks of 16; 85 / 61 / 27 fine chunks of 5 / 7 / 16 steps).
# A one-step last chunk and a last chunk of L - 1 steps, at (2, 2) and (3, 8)
# in the B = 70 and B = 230 forms.  (T = 417 would also be a one-step last
# chunk, but its 84 fine chunks of 5 steps fill algo 3's last unit at (3, 8).)
EXTRA_T = (401, 431)
# group mode without (J, d) at r = 3 needs B < 8, and 27 chunks of 3
# trajectories fit one 256-lane block: a second group needs more chunks
TWO_GROUPS = (7, 661)


def _cases():
    rows = []
    for si, (r, n) in enumerate(SHAPES):
        for fi, (form, (B, T, _)) in enumerate(FORMS.items()):
            E, dtype = SOURCES[(si + fi) % 3]
            rows.append((r, n, E, dtype, B, T, form))
            if (r, n) in ((2, 2), (3, 8)) and form in ("group_jd", "uniform"):
                for k, Tx in enumerate(EXTRA_T):
                    Ex, dx = SOURCES[(si + fi + 1 + k) % 3]
                    rows.append((r, n, Ex, dx, B, Tx, form))
        if (r, n) in ((3, 4), (3, 8)):
            E, dtype = SOURCES[si % 3]
            rows.append((r, n, E, dtype) + TWO_GROUPS + ("group",))
    return rows


# (r, n, E, dtype, B, T, expected form)
CASES = _cases()
IDS = [f"{r}x{n}-{form}-B{B}-T{T}-E{E}{dtype}" for r, n, E, dtype, B, T, form in CASES]


def _expected(r, form):
    want = dict(FORMS[form][2])
    if form == "group_jd" and r < 3:
        want["jd"] = 0
    return want


def _assert_form(r, n, E, B, T, form):
    """The built library's plan of this row: the form, and every raggedness
    condition.  Returns the algo-2 plan."""
    from eks_amd import _lib
    lib = _lib.load()
    tag = (r, n, E, B, T, form)
    assert lib.eks_smooth_algo(B, T, n, r, E, 2) == 2, tag
    assert lib.eks_smooth_algo(B, T, n, r, E, 3) == 3, tag
    p2 = _lib.plan_info(B, T, n, r, E, 2)
    assert p2["algo"] == 2, (tag, p2)
    got = {k: p2[k] for k in ("uniform_lanes", "wave_scan", "grp", "jd")}
    assert got == _expected(r, form), (tag, p2)
    if form == "wave":
        assert B > 256, tag
    assert p2["NC"] == -(-T // p2["L"]) and p2["NC"] > 1, (tag, p2)
    assert (p2["NC"] > 24) == bool(p2["wave_scan"]), (tag, p2)
    assert T % p2["L"] != 0 and T % p2["LS"] != 0, (tag, p2)
    assert p2["G"] == 1, (tag, p2)
    assert (p2["NG"] >= 1) == bool(p2["grp"]), (tag, p2)
    p3 = _lib.plan_info(B, T, n, r, E, 3)
    assert p3["algo"] == 3, (tag, p3)
    assert T % p3["fine_len3"] != 0, (tag, p3)
    assert p3["NCf"] == -(-T // p3["fine_len3"]) and p3["NCf"] % 4 != 0, (tag, p3)
    if r == 2:  # k3_fwd's units hold 8 fine chunks at r = 2
        assert p3["NCf"] % 8 != 0 and p3["NCu"] == -(-p3["NCf"] // 8), (tag, p3)
    assert p3["NCc"] == -(-p3["NCf"] // 4) and p3["ng"] == -(-B // 64), (tag, p3)
    return p2


def test_cases_stay_on_the_edges():
    """No GPU: every row takes the form it is in the table for and is ragged
    on every grid, as computed by the library's own plan functions; the table
    fills every shape x form cell and every form sees every member source."""
    for r, n, E, dtype, B, T, form in CASES:
        _assert_form(r, n, E, B, T, form)
    cells = {(r, n, form) for r, n, _, _, _, _, form in CASES}
    assert cells == set((r, n, f) for (r, n), f in itertools.product(SHAPES, FORMS))
    for form in FORMS:
        assert {(E, d) for _, _, E, d, _, _, f in CASES if f == form} == set(SOURCES), form
    for shape in SHAPES:
        assert {(E, d) for r, n, E, d, _, _, _ in CASES if (r, n) == shape} == set(SOURCES), shape
    from eks_amd import _lib
    # a one-step last chunk and one of L - 1 steps, in group and uniform mode
    for shape, form in itertools.product(((2, 2), (3, 8)), ("group_jd", "uniform")):
        last = set()  # lengths of the last chunk, as (steps, L)
        for r, n, E, _, B, T, f in CASES:
            if (r, n) == shape and f == form:
                L = _lib.plan_info(B, T, n, r, E, 2)["L"]
                last.add((T % L, L))
        assert any(k == 1 for k, L in last) and any(k == L - 1 for k, L in last), (shape, form, last)
    # group mode without (J, d) at r = 3 with more than one group per trajectory
    for shape in ((3, 4), (3, 8)):
        assert any(_lib.plan_info(B, T, n, r, E, 2)["NG"] > 1 for r, n, E, _, B, T, f in CASES
                   if (r, n) == shape and f == "group"), shape


# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _members(rng, r, n, E, dtype, B, T):
    """(B, E, T, n) float64 host copy of the members (float32 values for an
    f32 source; values no float32 holds for an f64 one)."""
    from eks_amd import synthetic
    if n == 2:
        st = synthetic.singleview_obs(rng, E, T, K=B)
    else:
        st = synthetic.multiview_obs(rng, n // 2, E, T, K=B)
    st = st.transpose(2, 0, 1, 3).astype(np.float64)
    if dtype == "f64":
        st = st + rng.normal(0.0, 1e-3, size=st.shape)
    return np.ascontiguousarray(st)


def _fit_models(stacks, n):
    from oracle import eks_oracle as O
    models = []
    for st in stacks:
        preds, ev = O.ensemble_array(st)
        p = (O.singleview_params if n == 2 else O.multicam_params)(preds, ev, 0.05, 25)
        models.append(dict(m0=p["m0"], S0=p["S0"], A=p["A"], Q=p["Q"], C=p["C"],
                           offset=p["means"]))
    return models


def _pack(models):
    from eks_amd import batch
    stk = lambda k: np.stack([m[k] for m in models])  # noqa: E731
    params = batch.pack_params(stk("m0"), stk("S0"), stk("A"), stk("Q"), stk("C"), stk("offset"))
    return params, batch.model_flags(stk("A"), stk("C"))


def _oracle(st, m):
    """out (T, n), ms (T, r) and the NLL of one trajectory, in float64 on the CPU."""
    from oracle import eks_oracle as O
    preds, ev = O.ensemble_array(st)
    y = preds - m["offset"]
    mf, Vf, S = O.filtering_pass(y, m["m0"], m["S0"], m["C"], np.eye(len(m["offset"])), m["A"],
                                 m["Q"], ev)
    ms, _, _ = O.smooth_backward(y, mf, Vf, S, m["A"])
    nll = O.compute_nll(y, m["m0"], m["S0"], m["C"], m["A"], m["Q"], ev)
    return ms @ m["C"].T + m["offset"], ms, nll


def _sample(B):
    """First and last lanes, both sides of a 64-trajectory group boundary."""
    return sorted({b for b in (0, 1, 63, 64, B // 2, B - 2, B - 1) if 0 <= b < B})


def _windows(T, L):
    return (("the last 2 L frames", slice(max(T - 2 * L, 0), T)),
            ("the first L frames", slice(0, min(L, T))),
            ("all frames", slice(0, T)))


def _run(batch, d, params, n, r, algo, flags):
    res = batch.smooth(d, params, n=n, r=r, algo=algo, flags=flags, want_nll=True, want_ms=True,
                       check=False)
    st = res["status"].cpu().numpy()
    assert (st == 0).all(), (f"algo {algo}: status != 0 on trajectories",
                             np.nonzero(st)[0][:8], st[st != 0][:8])
    return {k: res[k].cpu().numpy() for k in ("out", "ms", "nll")}


def _compare(got, ref, want, sample, T, L, what):
    """got / ref: algo a's and algo 1's results on all trajectories; want:
    {b: oracle (out, ms, nll)}.  Returns (max |out - algo 1|, max |out - oracle|)."""
    d_seq = d_orc = 0.0
    for name, win in _windows(T, L):
        if ref is not None:
            for key in ("out", "ms"):
                d = float(np.abs(got[key][:, win] - ref[key][:, win]).max())
                assert d < PX_ALGO, f"{what}: {key} differs from algo 1 by {d:.3e} in {name}"
                if key == "out":
                    d_seq = max(d_seq, d)
        for b in sample:
            out, ms, _ = want[b]
            d = float(np.abs(got["out"][b, win] - out[win]).max())
            assert d < OUT_TOL, f"{what}: out[{b}] differs from the oracle by {d:.3e} in {name}"
            d_orc = max(d_orc, d)
            try:
                _close(got["ms"][b, win], ms[win], rtol=INT_RTOL)
            except AssertionError as e:
                raise AssertionError(f"{what}: ms[{b}] differs from the oracle in {name}: {e}")
    if ref is not None:
        rel = float(np.abs((got["nll"] - ref["nll"]) / ref["nll"]).max())
        assert rel < NLL_RTOL, f"{what}: NLL differs from algo 1 by {rel:.3e} relative"
    for b in sample:
        nll = want[b][2]
        assert abs(got["nll"][b] - nll) <= NLL_ORACLE_RTOL * abs(nll), \
            f"{what}: NLL[{b}] = {got['nll'][b]!r}, oracle {nll!r}"
    return d_seq, d_orc


@pytest.mark.gpu
@pytest.mark.parametrize("r,n,E,dtype,B,T,form", CASES, ids=IDS)
def test_ragged_forms(torch, r, n, E, dtype, B, T, form):
    """One table row: algos 2 and 3 against algo 1 on every trajectory, all
    three against the oracle on the sample; whole trajectory, head and tail."""
    from eks_amd import _lib, batch
    plan = _assert_form(r, n, E, B, T, form)
    L = plan["L"]
    rng = np.random.default_rng(7000 + CASES.index((r, n, E, dtype, B, T, form)))
    stacks = _members(rng, r, n, E, dtype, B, T)
    models = _fit_models(stacks, n)
    params, flags = _pack(models)
    d = batch.make_time_major(stacks, dtype=np.float32 if dtype == "f32" else np.float64)
    sample = _sample(B)
    want = {b: _oracle(stacks[b], models[b]) for b in sample}
    lib = _lib.load()
    res = {}
    for a in (1, 2, 3):
        assert lib.eks_smooth_algo(B, T, n, r, E, a) == a
        res[a] = _run(batch, d, params, n, r, a, flags)
    worst = {}
    for a in (1, 2, 3):
        worst[a] = _compare(res[a], res[1] if a != 1 else None, want, sample, T, L,
                            f"{r}x{n} {form} B={B} T={T} algo {a}")
    print(f"RAGGED form={form} shape={r}x{n} B={B} T={T} "
          + " ".join(f"a{a}:d_algo1={worst[a][0]:.3e},d_oracle={worst[a][1]:.3e}" for a in worst))


SHORT_T = (1, 2, 3, 4, 5, 6, 7, 8, 9, 11)


@pytest.mark.gpu
@pytest.mark.parametrize("B", [3, 70])
@pytest.mark.parametrize("r,n", [(3, 4), (3, 8)])
def test_algo3_short_trajectories(torch, r, n, B):
    """algo 3 at r = 3 below one fine chunk, at exactly one, and below one
    unit (7-step fine chunks at (3, 4), 5-step at (3, 8); 4 per unit), with
    one exact-agreement frame (ev = 0) at t = 0 of trajectory 0."""
    from eks_amd import _lib, batch
    E, dtype = SOURCES[(n // 4 + B) % 3]
    T0 = 64                                   # the models are fitted on 64 frames
    rng = np.random.default_rng(900 + 10 * n + B)
    full = _members(rng, r, n, E, dtype, B, T0)
    full[0, :, 0, 0] = full[0, 0, 0, 0]       # all members equal: R_00 = 0 at t = 0
    models = _fit_models(full, n)
    params, flags = _pack(models)
    lib = _lib.load()
    fine = _lib.plan_info(B, 64, n, r, E, 3)["fine_len3"]
    assert min(SHORT_T) < fine and fine in SHORT_T and fine < max(SHORT_T) < 4 * fine
    for T in SHORT_T:
        assert lib.eks_smooth_algo(B, T, n, r, E, 3) == 3
        p3 = _lib.plan_info(B, T, n, r, E, 3)
        assert p3["algo"] == 3 and p3["NCf"] == -(-T // fine) and p3["NCc"] == 1
        stacks = np.ascontiguousarray(full[:, :, :T])
        d = batch.make_time_major(stacks, dtype=np.float32 if dtype == "f32" else np.float64)
        sample = sorted({0, B - 1})
        want = {b: _oracle(stacks[b], models[b]) for b in sample}
        r1 = _run(batch, d, params, n, r, 1, flags)
        r3 = _run(batch, d, params, n, r, 3, flags)
        _compare(r1, None, want, sample, T, T, f"{r}x{n} B={B} T={T} algo 1")
        _compare(r3, r1, want, sample, T, T, f"{r}x{n} B={B} T={T} algo 3")


@pytest.mark.gpu
@pytest.mark.parametrize("r,n", [(2, 2), (3, 8)])
def test_filter_only_ragged(torch, r, n):
    """Filter-only calls (batch.nll) of algo 2 at T = 421: they use chunk_len
    (not the smoothing calls' shorter chunks) and, with more than 24 chunks,
    the wave-parallel forward scan with the closed-form NLL shares."""
    from eks_amd import _lib, batch
    from oracle import eks_oracle as O
    T = 421
    for i, B in enumerate((5, 70, 260)):
        E, dtype = SOURCES[(n // 4 + i) % 3]
        plan = _lib.plan_info(B, T, n, r, E, 2, smoothing=False)
        assert plan["algo"] == 2 and plan["grp"] == 0 and plan["jd"] == 0, plan
        assert plan["NC"] > 24 and plan["wave_scan"] == 1 and T % plan["L"] != 0, plan
        rng = np.random.default_rng(500 + 10 * n + i)
        stacks = _members(rng, r, n, E, dtype, B, T)
        models = _fit_models(stacks, n)
        params, flags = _pack(models)
        d = batch.make_time_major(stacks, dtype=np.float32 if dtype == "f32" else np.float64)
        got = {}
        for a in (1, 2):
            status = torch.full((B,), -1, dtype=torch.int32, device="cuda")
            got[a] = batch.nll(d, params, n=n, r=r, algo=a, flags=flags, check=False,
                               status=status).cpu().numpy()
            assert (status.cpu().numpy() == 0).all(), (B, a)
        rel = float(np.abs((got[2] - got[1]) / got[1]).max())
        assert rel < NLL_RTOL, (B, rel)
        for b in _sample(B):
            m = models[b]
            preds, ev = O.ensemble_array(stacks[b])
            ref = O.compute_nll(preds - m["offset"], m["m0"], m["S0"], m["C"], m["A"], m["Q"], ev)
            for a in (1, 2):
                assert abs(got[a][b] - ref) <= NLL_ORACLE_RTOL * abs(ref), (B, b, a, got[a][b], ref)
