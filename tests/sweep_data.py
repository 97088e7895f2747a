"""Inputs and oracle references of the likelihood-sweep tests
(test_sweep_host.py, test_gpu_sweep.py): computed once per shape and shared,
read only.  The data follow tests/test_gpu_postvar.py's ``dataset``: seed
7 B + T, E = 5 float32 members, models from the oracle with smooth_param = 1."""
import functools

import numpy as np

SCALES = tuple(10.0 ** e for e in range(-3, 4))  # the candidates: Q x {1e-3 .. 1e3}, K = 7
PUPIL_A = (.9999, .999, .999)


def model_of(kind, stack, A=PUPIL_A):
    from oracle import eks_oracle as O
    preds, ev = O.ensemble_array(stack)
    if kind == "sv":
        return O.singleview_params(preds, ev, 1.0, 50.0)
    if kind == "mc":
        return O.multicam_params(preds, ev, 1.0, 25.0)
    return O.pupil_params(preds, np.diag(A))


def oracle_nll(stack, p, s=1.0, mode="median"):
    """compute_nll of the model ``p`` with Q scaled by s on the members (E, T, n)."""
    from oracle import eks_oracle as O
    preds, ev = O.ensemble_array(stack, mode)
    return O.compute_nll(preds - p["means"], p["m0"], p["S0"], p["C"], p["A"], s * p["Q"], ev)


@functools.lru_cache(maxsize=None)
def dataset(kind, B, T, V=4, E=5):
    """(members (B, E, T, n) float32-exact float64, models, oracle NLL (K, B))."""
    from eks_amd import synthetic
    rng = np.random.default_rng(7 * B + T)
    if kind == "sv":
        st = synthetic.singleview_obs(rng, E, T, K=B).transpose(2, 0, 1, 3)
    elif kind == "mc":
        st = synthetic.multiview_obs(rng, V, E, T, K=B).transpose(2, 0, 1, 3)
    else:
        st = np.stack([synthetic.pupil_obs(rng, E, T) for _ in range(B)])
    st = st.astype(np.float64)
    models = [model_of(kind, st[b]) for b in range(B)]
    ref = np.array([[oracle_nll(st[b], models[b], s) for b in range(B)] for s in SCALES])
    st.setflags(write=False)
    ref.setflags(write=False)
    return st, models, ref


def candidate_rows(models, scales=SCALES):
    """(K, B) models as numpy (K * B, P) rows: row k * B + b = candidate k of trajectory b."""
    rows = []
    for s in scales:
        for m in models:
            rows.append(np.concatenate([m["m0"].ravel(), m["S0"].ravel(), m["A"].ravel(),
                                        (s * m["Q"]).ravel(), m["C"].ravel(), m["means"].ravel()]))
    return np.stack(rows)
