"""The private helpers every entry point of eks_amd/batch.py opens with, on CPU
tensors: the member input (a view of any strides or a Yev), the plane layout
of a Yev against eks_yev_bytes, and the reuse of a Yev's buffer.  Nothing here
needs a device."""
import pytest

torch = pytest.importorskip("torch")

from eks_amd import _lib, batch  # noqa: E402


@pytest.mark.parametrize("dtype,code", [(torch.float32, _lib.EKS_F32), (torch.float64, _lib.EKS_F64)])
def test_member_input_of_a_permuted_view(dtype, code):
    B, T, E, n = 3, 5, 4, 2
    obs = torch.zeros((T, E, n, B), dtype=dtype).permute(3, 0, 1, 2)  # viewed as (B, T, E, n)
    i = batch._member_input(obs, n, "mean")
    assert (i.ptr, i.code, i.B, i.T, i.E) == (obs.data_ptr(), code, B, T, E)
    assert i.strides == (1, E * n * B, n * B, B) and i.mode == _lib.EKS_MEAN
    assert batch._member_input(obs, n, "median", members_only=True).mode == _lib.EKS_MEDIAN
    assert batch._member_input(obs, n, None).mode is None  # an entry point without a mode


def test_member_input_of_a_yev():
    B, T, E, n = 3, 5, 4, 2
    buf = torch.zeros(batch.Yev.layout(B, T, n, _lib.EKS_YEV32)[2], dtype=torch.uint8)
    yev = batch.Yev(buf, B, T, E, n, _lib.EKS_YEV32, "mean")
    i = batch._member_input(yev, n, "mean")
    assert i == (buf.data_ptr(), _lib.EKS_YEV32, B, T, E, (0, 0, 0, 0), _lib.EKS_MEAN)
    assert batch._member_input(yev, n, None).mode is None
    with pytest.raises(ValueError, match="another averaging mode"):
        batch._member_input(yev, n, "median")
    with pytest.raises(ValueError, match="obs has 2 coordinates, expected n=8"):
        batch._member_input(yev, 8, "mean")
    with pytest.raises(TypeError, match="member view"):
        batch._member_input(yev, n, "mean", members_only=True)


def test_member_input_rejects():
    obs = torch.zeros((3, 5, 4, 2))
    with pytest.raises(ValueError, match=r"obs must be viewed as \(B, T, E, n\)"):
        batch._member_input(obs[0], 2, "median")
    with pytest.raises(ValueError, match="obs has 2 coordinates, expected n=3"):
        batch._member_input(obs, 3, "median")
    with pytest.raises(TypeError, match="obs must be float32 or float64"):
        batch._member_input(obs.to(torch.float16), 2, "median")
    with pytest.raises(ValueError, match="mode7 averaging not supported"):
        batch._member_input(obs, 2, "mode7")


def test_params_and_status_checks():
    P = batch.param_len(2, 2)
    batch._check_params(torch.zeros((6, P), dtype=torch.float64), 6, 2, 2)
    for bad in (torch.zeros((5, P), dtype=torch.float64), torch.zeros((6, P)),
                torch.zeros((P, 6), dtype=torch.float64).t()):
        with pytest.raises(ValueError, match=rf"params must be a contiguous \(6, {P}\) float64"):
            batch._check_params(bad, 6, 2, 2)
    with pytest.raises(ValueError, match="params must be"):  # K < 0
        batch._check_params(torch.zeros((0, P), dtype=torch.float64), 0, 2, 2, ok=False)
    st = torch.zeros((2, 3), dtype=torch.int32)
    assert batch._status_words(st, (2, 3), "cpu") is st
    new = batch._status_words(None, (3,), "cpu")
    assert new.shape == (3,) and new.dtype == torch.int32
    for bad in (st, torch.zeros((3,), dtype=torch.int64), torch.zeros((6,), dtype=torch.int32)[::2]):
        with pytest.raises(ValueError, match=r"status must be a contiguous \(3,\) int32 tensor"):
            batch._status_words(bad, (3,), "cpu")


# (3, 5, 2): the float32 y planes end at byte 120 and ev starts at 256, so the
# padding matters; (8, 8, 1): the float64 y planes end on 512, no padding
@pytest.mark.parametrize("B,T,n", [(3, 5, 2), (8, 8, 1)])
@pytest.mark.parametrize("code,dt,ydtype,ysize", [(_lib.EKS_YEV32, _lib.EKS_F32, torch.float32, 4),
                                                  (_lib.EKS_YEV64, _lib.EKS_F64, torch.float64, 8)])
def test_yev_planes_against_eks_yev_bytes(B, T, n, code, dt, ydtype, ysize):
    lib = _lib.load()
    E = 3  # (median of 3 float32 members: float32 planes)
    assert lib.eks_yev_dtype(dt, E, _lib.EKS_MEDIAN) == code
    nbytes = lib.eks_yev_bytes(B, T, n, dt, E, _lib.EKS_MEDIAN)
    ybytes, ev_off, end = batch.Yev.layout(B, T, n, code)
    assert ybytes == T * n * B * ysize and ev_off % 256 == 0 and 0 <= ev_off - ybytes < 256
    assert end == ev_off + T * n * B * 8 == nbytes
    if (B, T, n, ysize) == (3, 5, 2, 4):
        assert (ybytes, ev_off) == (120, 256)
    if (B, T, n, ysize) == (8, 8, 1, 8):
        assert ybytes == ev_off == 512
    buf = torch.zeros(nbytes, dtype=torch.uint8)
    y, ev = batch.Yev(buf, B, T, E, n, code, "median").planes()
    assert y.shape == ev.shape == (T, n, B) and y.dtype == ydtype and ev.dtype == torch.float64
    assert y.is_contiguous() and ev.is_contiguous()
    # where the views start and end in the buffer: disjoint, ev last, ending at eks_yev_bytes
    y0, ev0 = y.data_ptr() - buf.data_ptr(), ev.data_ptr() - buf.data_ptr()
    assert (y0, y0 + y.numel() * ysize) == (0, ybytes)
    assert (ev0, ev0 + ev.numel() * 8) == (ev_off, nbytes) and ev0 >= ybytes
    # plane (t, j) holds the B trajectories side by side, and the views alias the buffer
    y[1, n - 1, 2] = 1.0
    ev[T - 1, 0, B - 1] = 2.0
    assert int((buf != 0).sum()) > 0 and buf[ybytes:ev_off].sum() == 0
    assert buf[:ybytes].view(ydtype)[(1 * n + n - 1) * B + 2] == 1.0
    assert buf[ev_off:].view(torch.float64)[((T - 1) * n) * B + B - 1] == 2.0


def test_yev_reuse():
    shape, code = (3, 5, 4, 2), _lib.EKS_YEV64
    nbytes = batch.Yev.layout(3, 5, 2, code)[2]
    new = batch._yev_out(True, shape, code, "median", nbytes, "cpu")
    assert (new.shape, new.code, new.mode) == (shape, code, "median")
    assert new.buf.numel() == nbytes and new.buf.dtype == torch.uint8
    # the same form: the very object; another shape, code or mode: its buffer, a new header
    assert batch._yev_out(new, shape, code, "median", nbytes, "cpu") is new
    for shp, c, mode in [((3, 4, 4, 2), code, "median"), (shape, _lib.EKS_YEV32, "median"),
                         (shape, code, "mean")]:
        again = batch._yev_out(new, shp, c, mode, nbytes - 8, "cpu")
        assert again is not new and again.buf is new.buf
        assert (again.shape, again.code, again.mode, again.B, again.T) == (shp, c, mode, 3, shp[1])
    assert (new.shape, new.code, new.mode) == (shape, code, "median")  # the old header is not touched
    # too small: a new buffer
    bigger = batch._yev_out(new, (4, 5, 4, 2), code, "median", nbytes + 1, "cpu")
    assert bigger.buf is not new.buf and bigger.buf.numel() == nbytes + 1 and bigger.B == 4
    assert batch._yev_out(None, shape, code, "median", 0, "cpu").buf.numel() == 1
