"""The argument contract of the five chunked-scan entry points (eks_smooth_var,
eks_smooth_gaps, eks_nll_sweep, eks_nll_sweep_gaps, eks_draws_gaps) as one
table: from one valid call at B=3, T=10, E=4, n=2, r=2 every row changes one
argument and names the return code; the message must name the entry point.
The codes were recorded from the library before the entry points shared their
argument check (host_api.hpp), so the table pins that the shared check
answers as the five copies did.  A second table does the same for the entry
points' own checks (K, S, pvar without out) and pins where they stand in the
order.  Every row fails before a launch: no kernel runs and no pointer is
dereferenced."""
import ctypes

import pytest

from eks_amd import _lib

ARG, UNSUP = _lib.EKS_ERR_ARG, _lib.EKS_ERR_UNSUPPORTED
B, T, E, N, R, K, S = 3, 10, 4, 2, 2, 2, 2
PTR = 8  # a non-NULL address that is never read

# the arguments of each entry point in header order: (name, value of the valid call);
# "ws_bytes" is filled in from the entry point's own workspace query
_MEMBERS = [("obs", PTR), ("dtype", _lib.EKS_F32), ("B", B), ("T", T), ("E", E), ("n", N), ("r", R),
            ("sb", 0), ("st", 0), ("se", 0), ("sj", 0)]
_TAIL = [("ws", PTR), ("ws_bytes", None), ("status", PTR), ("stream", 0)]
_OUT = [("out", PTR), ("ob", 0), ("ot", 0), ("oj", 0)]
ENTRIES = {
    "eks_smooth_var": dict(
        args=_MEMBERS + [("params", PTR), ("pvar", PTR), ("vb", 0), ("vt", 0), ("vj", 0), ("Vs", 0)]
        + _TAIL,
        pointers=("obs", "params", "pvar", "status"),
        need=lambda lib: lib.eks_smooth_var_workspace_bytes(B, T, N, R)),
    "eks_smooth_gaps": dict(
        args=_MEMBERS + [("mode", _lib.EKS_MEDIAN), ("params", PTR)] + _OUT
        + [("pvar", 0), ("ms", 0), ("Vs", 0), ("nll", 0), ("nobs", 0)] + _TAIL,
        pointers=("obs", "params", "out", "status"),
        need=lambda lib: lib.eks_smooth_gaps_workspace_bytes(B, T, N, R)),
    "eks_nll_sweep": dict(
        args=_MEMBERS + [("mode", _lib.EKS_MEDIAN), ("params", PTR), ("K", K), ("nll", PTR)] + _TAIL,
        pointers=("obs", "params", "nll", "status"),
        need=lambda lib: lib.eks_nll_sweep_workspace_bytes(B, K, T, N, R)),
    "eks_nll_sweep_gaps": dict(
        args=_MEMBERS + [("mode", _lib.EKS_MEDIAN), ("params", PTR), ("K", K), ("nll", PTR),
                         ("nobs", 0)] + _TAIL,
        pointers=("obs", "params", "nll", "status"),
        need=lambda lib: lib.eks_nll_sweep_gaps_workspace_bytes(B, K, T, N, R)),
    "eks_draws_gaps": dict(
        args=_MEMBERS + [("mode", _lib.EKS_MEDIAN), ("params", PTR), ("S", S), ("noise", 0),
                         ("zb", 0), ("zs", 0), ("zt", 0), ("seed", 1), ("draws", PTR), ("db", 0),
                         ("ds", 0), ("dt", 0), ("dj", 0), ("xdraws", 0)] + _OUT + [("pvar", 0)]
        + _TAIL,
        pointers=("obs", "params", "draws", "status"),
        need=lambda lib: lib.eks_draws_gaps_workspace_bytes(B, S, T, N, R)),
}

# (row name, the changed arguments, return code); ws_bytes="short" is one byte under the need
ROWS = [
    ("T=0", dict(T=0), ARG),
    ("E=0", dict(E=0), ARG),
    ("dtype 9", dict(dtype=9), ARG),
    ("mode 7", dict(mode=7), ARG),
    ("r=4", dict(r=4), UNSUP),
    ("n=65", dict(n=65), UNSUP),
    ("E = max + 1", dict(E="max+1"), UNSUP),
    ("no workspace", dict(ws=0), ARG),
    ("workspace one byte short", dict(ws_bytes="short"), ARG),
]


def _call(lib, name, **changed):
    spec = ENTRIES[name]
    need = spec["need"](lib)
    assert need > 0
    vals = dict(spec["args"], ws_bytes=need)
    for k, v in changed.items():
        assert k in vals, (name, k)
        vals[k] = {"max+1": lib.eks_max_members() + 1, "short": need - 1}.get(v, v)
    types = _lib.SIGNATURES[name][1]
    assert len(types) == len(spec["args"])
    args = [(vals[k] or None) if t is ctypes.c_void_p else vals[k]
            for (k, _), t in zip(spec["args"], types)]
    return getattr(lib, name)(*args)


def _cases():
    for name, spec in ENTRIES.items():
        for p in spec["pointers"]:
            yield name, f"{p} NULL", {p: 0}, ARG
        for row, changed, code in ROWS:
            if all(k in dict(spec["args"]) for k in changed):  # eks_smooth_var has no mode
                yield name, row, changed, code


@pytest.mark.parametrize("name,row,changed,code", [pytest.param(*c, id=f"{c[0]}-{c[1]}")
                                                   for c in _cases()])
def test_one_bad_argument(name, row, changed, code):
    lib = _lib.load()
    assert _call(lib, name, **changed) == code
    msg = lib.eks_last_error().decode()
    assert msg.startswith(name + ":"), msg
    if "NULL" in row:
        assert "NULL" in msg
    if "workspace" in row:
        assert "workspace" in msg
    if row == "dtype 9":
        assert "dtype" in msg


# The entry points' own checks (K, S, pvar without out) and their place in the
# order: after the sizes, before the dtype and the mode.  (entry point, the
# changed arguments, words of the message that must win)
_SWEEP_OWN = [(dict(K=-1), "K>=0"), (dict(K=-1, dtype=9), "K>=0"), (dict(K=-1, mode=7), "K>=0"),
              (dict(K=-1, T=0), "T>=1"), (dict(K=-1, obs=0), "NULL")]
OWN_ROWS = [(name, *row) for name in ("eks_nll_sweep", "eks_nll_sweep_gaps") for row in _SWEEP_OWN]
OWN_ROWS += [("eks_draws_gaps", *row) for row in [
    (dict(S=-1), "S>=0"), (dict(S=-1, dtype=9), "S>=0"), (dict(S=-1, T=0), "T>=1"),
    (dict(S=-1, status=0), "NULL"), (dict(pvar=PTR, out=0), "pass out"),
    (dict(pvar=PTR, out=0, S=-1), "S>=0"), (dict(pvar=PTR, out=0, mode=7), "pass out"),
    (dict(pvar=PTR, out=0, dtype=9), "pass out"), (dict(pvar=PTR, out=0, E=0), "E>=1")]]


@pytest.mark.parametrize("name,changed,words", OWN_ROWS,
                         ids=[f"{n}-{'-'.join(c)}" for n, c, _ in OWN_ROWS])
def test_own_checks_and_their_place(name, changed, words):
    lib = _lib.load()
    assert _call(lib, name, **changed) == ARG
    msg = lib.eks_last_error().decode()
    assert msg.startswith(name + ":") and words in msg, msg


def test_the_table_is_complete():
    names = [c[0] for c in _cases()]
    # 4 pointers + 9 rows each; eks_smooth_var has no averaging mode
    assert {n: names.count(n) for n in ENTRIES} == {
        "eks_smooth_var": 12, "eks_smooth_gaps": 13, "eks_nll_sweep": 13,
        "eks_nll_sweep_gaps": 13, "eks_draws_gaps": 13}
