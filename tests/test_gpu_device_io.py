"""Device-resident I/O (tomo_set_*_device / tomo_get_*_device, k_io_in / k_io_out): torch tensors on the GPU in and out of the
engine without a host trip.  Everything here is a copy or one correctly rounded conversion, so every comparison is bit for bit.

Shapes (Nslice, Nray, Nangles) are the smallest at which the kernels can go wrong: one slice and one angle; odd sizes (the scalar
path: rows that are no multiple of four); past one 32-slice tile; angles past one 32-column tile with two 64-slice chunks; three
chunks; four chunks.  Volume rows (Nray^2) and sinogram rows (Nray * Nangles) give both the 16-byte and the scalar form."""
import ctypes

import numpy as np
import pytest
import torch

from local_ring import ThreadRing
from tomo_tv_amd import _lib, pytvlib
from tomo_tv_amd._lib import (F32, F64, S_COUNT, SINO_B, SINO_G, SINO_PACKED, SINO_PUBLIC, SINO_USER0, VOL_ORIGINAL, VOL_RECON, VOL_USER0,
                              VOL_YK)
from tomo_tv_amd.distributed import slab_partition
from tomo_tv_amd.engine import _on_device, _ptr, tomoengine
from tomo_tv_amd.reconstructor import TomoGPU

pytestmark = pytest.mark.gpu
SHAPES = [(1, 8, 1), (3, 9, 5), (33, 16, 5), (65, 40, 33), (130, 32, 7), (256, 16, 3)]
IDS = ["x".join(map(str, s)) for s in SHAPES]
DEV = torch.device("cuda", 0)
TDT = {F32: torch.float32, F64: torch.float64}
ERR_ARG = 1
_engines = {}


def angles(P):
    return np.linspace(-60.0, 60.0, P) * np.pi / 180


def engine(shape):
    """One engine per shape for the whole module (every test sets what it reads)."""
    if shape not in _engines:
        nx, n, P = shape
        _engines[shape] = tomoengine(nx, n, angles(P), device=0)
    return _engines[shape]


def values32(shape, seed):
    """float32, every element distinct, both signs"""
    n = int(np.prod(shape))
    rng = np.random.default_rng(seed)
    a = ((rng.permutation(n).astype(np.float64) - n // 2) * 0.37 + 0.11).astype(np.float32).reshape(shape)
    assert np.unique(a).size == n and (a < 0).any() and (a > 0).any()
    return a


def values64(shape, seed):
    """float64 between neighbouring float32 values, a quarter, a half (ties) and three quarters of the way: values whose nearest-even
    float32 differs from the truncated one; and the float32 they must become"""
    base = values32(shape, seed)
    frac = np.resize(np.array([0.25, 0.5, 0.75, 0.0]), base.size).reshape(shape)
    a = base.astype(np.float64) + frac * np.spacing(base).astype(np.float64)
    want = a.astype(np.float32)
    trunc = np.where(np.abs(want.astype(np.float64)) > np.abs(a), np.nextafter(want, np.float32(0)), want)
    assert (trunc != want).mean() > 0.2 or base.size < 8          # rounding up happened: truncation would give other bits
    return a, want


def inputs(shape, dtype, seed):
    """(array to hand over in `dtype`, the float32 content the engine must then hold)"""
    if dtype == F64:
        return values64(shape, seed)
    a = values32(shape, seed)
    return a, a


def host_get_volume(t, which):
    out = np.empty((t.nloc, t.Ny, t.Nz), np.float32)
    t.be.c("get_volume", which, _ptr(out))
    return out


def host_get_sino(t, which):
    out = np.empty((t.nloc, t.Nrow), np.float32)
    t.be.c("get_sinogram", which, _ptr(out))
    return out


def same(got, want):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    bad = np.argwhere(got != want)
    assert got.shape == want.shape and got.dtype == want.dtype and len(bad) == 0, (len(bad), bad[:4].tolist())


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_volume_round_trips(gpu, shape, dtype):
    nx, n, _ = shape
    t = engine(shape)
    for k, slot in enumerate((VOL_RECON, VOL_USER0 + 1)):
        a, want = inputs((nx, n, n), dtype, 10 + k)
        t.set_volume_tensor(torch.from_numpy(a).to(DEV), slot)                   # set by device, get by host
        same(host_get_volume(t, slot), want)
        h = values32((nx, n, n), 20 + k)
        t.be.c("set_volume", slot, _ptr(h))                                      # set by host, get by device
        got = t.get_volume_tensor(slot, dtype=TDT[dtype])
        assert got.device == DEV and got.dtype == TDT[dtype]
        same(got, h.astype(np.float64) if dtype == F64 else h)


@pytest.mark.parametrize("layout", [SINO_PACKED, SINO_PUBLIC], ids=["packed", "public"])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_sinogram_round_trips(gpu, shape, dtype, layout):
    nx, n, P = shape
    t = engine(shape)
    a, want = inputs((nx, n, P), dtype, 30)                                      # public layout
    packed = pytvlib.pack_tilt_series(want)
    give = a if layout == SINO_PUBLIC else pytvlib.pack_tilt_series(a)
    t.set_tilt_series_tensor(torch.from_numpy(give).to(DEV), layout)             # set by device, get by host
    got_dev = host_get_sino(t, SINO_B)
    same(got_dev, packed)
    t.set_tilt_series(packed)                                                    # the host path: pack_tilt_series + set_tilt_series
    same(got_dev, host_get_sino(t, SINO_B))
    h = values32((nx, n, P), 31)
    t.be.c("set_sinogram", SINO_USER0, _ptr(pytvlib.pack_tilt_series(h)))        # set by host, get by device
    got = t.get_projections_tensor(SINO_USER0, layout, dtype=TDT[dtype])
    ref = h if layout == SINO_PUBLIC else pytvlib.pack_tilt_series(h)
    assert got.device == DEV
    same(got, ref.astype(np.float64) if dtype == F64 else ref)


def _descend(t):
    """one SART sweep, two TV descent steps, the data distance: volumes and every scalar"""
    t.initialize_SART("sequential")
    t.SART(0.7, 1)
    tv = t.tv_gd(2, 0.05)
    dd = t.data_distance()
    return host_get_volume(t, VOL_RECON), host_get_sino(t, SINO_G), t.be.scalars(), tv, dd


@pytest.mark.parametrize("shape", [(33, 16, 5), (130, 32, 7)], ids=["33x16x5", "130x32x7"])
def test_padding_slices_are_written_as_zero(gpu, shape):
    """Slots that earlier work has filled (a tilt series, three SIRT iterations) are set again, by device on one engine and by host on
    another: the sweeps, stencils and reductions that run over the padded width give the same volumes and scalars bit for bit."""
    nx, n, P = shape
    b0, x1, b1 = np.abs(values32((nx, n, P), 40)), np.abs(values32((nx, n, n), 41)) * 1e-3, np.abs(values32((nx, n, P), 42))
    out = []
    for by_device in (True, False):
        t = tomoengine(nx, n, angles(P), device=0)
        t.set_tilt_series(pytvlib.pack_tilt_series(b0))
        t.initialize_SIRT()
        t.SIRT(3)
        assert host_get_volume(t, VOL_RECON).any()
        if by_device:
            t.set_volume_tensor(torch.from_numpy(x1).to(DEV), VOL_RECON)
            t.set_tilt_series_tensor(torch.from_numpy(b1).to(DEV), SINO_PUBLIC)
        else:
            t.set_volume(x1, VOL_RECON)
            t.set_tilt_series(pytvlib.pack_tilt_series(b1))
        out.append(_descend(t))
    (xv, gv, sv, tvv, ddv), (xh, gh, sh, tvh, ddh) = out
    same(xv, xh)
    same(gv, gh)
    assert np.array_equal(sv, sh) and sv.shape == (S_COUNT,), (sv, sh)
    assert tvv == tvh and ddv == ddh and ddv > 0 and tvv > 0


@pytest.mark.parametrize("pad", [64, 3], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("shape", [(3, 9, 5), (33, 16, 5), (65, 40, 33)], ids=["3x9x5", "33x16x5", "65x40x33"])
def test_getters_write_nothing_outside_their_elements(gpu, shape, dtype, pad):
    nx, n, P = shape
    t = engine(shape)
    x, b = values32((nx, n, n), 50), values32((nx, n, P), 51)
    t.be.c("set_volume", VOL_RECON, _ptr(x))
    t.be.c("set_sinogram", SINO_USER0, _ptr(pytvlib.pack_tilt_series(b)))
    sentinel = -12345.5
    cast = (lambda a: a.astype(np.float64)) if dtype == F64 else (lambda a: a)
    for want, get in ((x, lambda o: t.get_volume_tensor(VOL_RECON, out=o)),
                      (b, lambda o: t.get_projections_tensor(SINO_USER0, SINO_PUBLIC, out=o)),
                      (pytvlib.pack_tilt_series(b), lambda o: t.get_projections_tensor(SINO_USER0, SINO_PACKED, out=o))):
        big = torch.full((want.size + 2 * pad,), sentinel, dtype=TDT[dtype], device=DEV)
        inner = big[pad:pad + want.size].view(want.shape)
        assert get(inner) is inner
        host = big.cpu().numpy()
        assert (host[:pad] == sentinel).all() and (host[pad + want.size:] == sentinel).all()
        same(host[pad:pad + want.size].reshape(want.shape), cast(want))


def _keep_busy(x, rounds=200):
    for _ in range(rounds):
        x.mul_(1.0001)


def test_set_is_ordered_behind_the_callers_stream(gpu):
    """On a side stream: a long run of kernels, then the fill of the input tensor, then the set -- no host synchronisation in between:
    the engine must read the filled tensor, not what it held when the call was made."""
    shape = (65, 40, 33)
    nx, n, P = shape
    t = engine(shape)
    x, b = values32((nx, n, n), 60), values32((nx, n, P), 61)
    xs, bs = torch.from_numpy(x).to(DEV), torch.from_numpy(b).to(DEV)
    xin, bin_, busy = torch.zeros_like(xs), torch.zeros_like(bs), torch.ones(1 << 26, device=DEV)
    side = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize(DEV)
    with torch.cuda.stream(side):
        _keep_busy(busy)
        xin.copy_(xs)
        bin_.copy_(bs)
        t.set_volume_tensor(xin, VOL_USER0)
        t.set_tilt_series_tensor(bin_, SINO_PUBLIC)
        xin.zero_()                                   # and the caller may reuse its buffer at once, on its stream
        bin_.zero_()
    same(host_get_volume(t, VOL_USER0), x)            # (the host getters wait for the engine's stream only)
    same(host_get_sino(t, SINO_B), pytvlib.pack_tilt_series(b))


def test_get_orders_the_callers_stream_behind_the_engine(gpu):
    """The mirror: the engine is busy (SIRT iterations queued on its stream) when the get is enqueued; the side stream consumes the
    tensor right after the call and must see the engine's data, not the sentinel it had filled the tensor with."""
    shape = (65, 40, 33)
    nx, n, P = shape
    t = engine(shape)
    b = np.abs(values32((nx, n, P), 62))
    t.set_tilt_series(pytvlib.pack_tilt_series(b))
    t.restart_recon()
    t.initialize_SIRT()
    side = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize(DEV)
    with torch.cuda.stream(side):
        out = torch.full((nx, n, n), -7.0, device=DEV)
        t.SIRT(40)
        t.get_volume_tensor(VOL_RECON, out=out)
        copy = out.clone()
    side.synchronize()
    want = host_get_volume(t, VOL_RECON)
    assert want.any() and (want >= 0).all()
    same(copy, want)


def test_refusals(gpu):
    shape = (33, 16, 5)
    nx, n, P = shape
    t = engine(shape)
    x = values32((nx, n, n), 70)
    t.be.c("set_volume", VOL_RECON, _ptr(x))
    # in Python, before any C call
    with pytest.raises(ValueError, match="CPU"):
        t.set_volume_tensor(torch.from_numpy(x))
    with pytest.raises(ValueError, match="CPU"):
        t.set_tilt_series_tensor(torch.zeros(nx, n, P), SINO_PUBLIC)
    with pytest.raises(ValueError, match="CPU"):
        t.get_volume_tensor(out=torch.empty(nx, n, n))
    good = torch.from_numpy(x).to(DEV)
    with pytest.raises(ValueError, match="cuda:0"):
        _on_device(good, 1)
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError, match="cuda:1"):
            t.set_volume_tensor(good.to("cuda:1"))
    with pytest.raises(ValueError, match="slices"):
        t.set_volume_tensor(good[:-1])
    with pytest.raises(ValueError, match="shape"):
        t.set_volume_tensor(good[:, :-1])
    # at the C level: TOMO_ERR_ARG with a message, nothing launched
    L, h, st = t.be.L, t.be.h, ctypes.c_void_p(0)
    p, nv, ns = ctypes.c_void_p(good.data_ptr()), nx * n * n, nx * n * P
    sino = torch.zeros(nx, n, P, device=DEV)
    q = ctypes.c_void_p(sino.data_ptr())
    pinned = torch.zeros(max(nv, ns)).pin_memory()
    pin = ctypes.c_void_p(pinned.data_ptr())
    calls = [
        ("nelems", lambda: L.tomo_set_volume_device(h, VOL_RECON, p, F32, nv - 1, st)),
        ("nelems", lambda: L.tomo_get_volume_device(h, VOL_RECON, p, F32, nv + 1, st)),
        ("nelems", lambda: L.tomo_set_sinogram_device(h, SINO_B, q, F32, SINO_PUBLIC, ns + n, st)),
        ("nelems", lambda: L.tomo_get_sinogram_device(h, SINO_B, q, F32, SINO_PACKED, 0, st)),
        ("null", lambda: L.tomo_set_volume_device(h, VOL_RECON, None, F32, nv, st)),
        ("null", lambda: L.tomo_get_volume_device(h, VOL_RECON, None, F32, nv, st)),
        ("null", lambda: L.tomo_set_sinogram_device(h, SINO_B, None, F32, SINO_PUBLIC, ns, st)),
        ("null", lambda: L.tomo_get_sinogram_device(h, SINO_B, None, F32, SINO_PUBLIC, ns, st)),
        ("dtype", lambda: L.tomo_set_volume_device(h, VOL_RECON, p, 2, nv, st)),
        ("dtype", lambda: L.tomo_get_sinogram_device(h, SINO_B, q, -1, SINO_PUBLIC, ns, st)),
        ("layout", lambda: L.tomo_set_sinogram_device(h, SINO_B, q, F32, 2, ns, st)),
        ("layout", lambda: L.tomo_get_sinogram_device(h, SINO_B, q, F32, -1, ns, st)),
        ("device memory", lambda: L.tomo_set_volume_device(h, VOL_RECON, pin, F32, nv, st)),
        ("device memory", lambda: L.tomo_get_volume_device(h, VOL_RECON, pin, F32, nv, st)),
        ("device memory", lambda: L.tomo_set_sinogram_device(h, SINO_B, pin, F32, SINO_PUBLIC, ns, st)),
        ("device memory", lambda: L.tomo_get_sinogram_device(h, SINO_B, pin, F32, SINO_PACKED, ns, st)),
        ("volume id", lambda: L.tomo_set_volume_device(h, 10 ** 6, p, F32, nv, st)),
        ("sinogram id", lambda: L.tomo_set_sinogram_device(h, _lib.SINO_YK_MODEL, q, F32, SINO_PUBLIC, ns, st)),
    ]
    for what, call in calls:
        assert call() == ERR_ARG, what
        assert what in L.tomo_last_error().decode(), (what, L.tomo_last_error())
    torch.cuda.synchronize(DEV)
    assert not pinned.any() and not sino.any()
    same(good, x)
    same(host_get_volume(t, VOL_RECON), x)


def test_device_calls_allocate_no_staging_buffer(gpu):
    nx, n, P = 33, 16, 5
    t = tomoengine(nx, n, angles(P), device=0)
    assert t.get_option("stage_bytes") == 0
    x, b = values32((nx, n, n), 80), values32((nx, n, P), 81)
    t.set_volume_tensor(torch.from_numpy(x).to(DEV), VOL_RECON)
    t.set_tilt_series_tensor(torch.from_numpy(b).to(DEV), SINO_PUBLIC)
    same(t.get_volume_tensor(VOL_RECON), x)
    same(t.get_projections_tensor(SINO_B, SINO_PUBLIC, dtype=torch.float64), b.astype(np.float64))
    assert t.get_option("stage_bytes") == 0
    same(host_get_volume(t, VOL_RECON), x)
    assert t.get_option("stage_bytes") == nx * n * n * 4


def _fista_iterations(t, count, t0, lam=0.05):
    dd = []
    for _ in range(count):
        pytvlib.run(t, "fista")
        t.tv_fgp(3, lam, vol=VOL_YK)
        tk = 0.5 * (1 + np.sqrt(1 + 4 * t0 ** 2))
        t.fista_momentum((t0 - 1) / tk)
        t0 = tk
        dd.append(t.data_distance())
        t.fista_project_yk()
    return t0, dd


def test_a_device_set_invalidates_what_a_host_set_invalidates(gpu):
    """FISTA with momentum leaves claims behind (recon_old == recon as a flag, the model sinogram as A * recon, A * yk by linearity);
    setting RECON must drop them, by device as by host: the cost of the new point and the next iteration are the same bit for bit."""
    nx, n, P = 33, 16, 5
    b = np.abs(values32((nx, n, P), 90)) * 1e-2
    x1 = np.abs(values32((nx, n, n), 91)) * 1e-4
    res = []
    for mode in ("device", "host"):
        t = tomoengine(nx, n, angles(P), device=0)
        t.set_tilt_series(pytvlib.pack_tilt_series(b))
        pytvlib.initialize_algorithm(t, "fista")
        t0, _ = _fista_iterations(t, 2, 1.0)
        if mode == "device":
            t.set_volume_tensor(torch.from_numpy(x1).to(DEV), VOL_RECON)
        else:
            t.set_volume(x1, VOL_RECON)
        first_dd = t.data_distance()
        _, dd = _fista_iterations(t, 1, t0)
        res.append((first_dd, dd, host_get_volume(t, VOL_RECON), host_get_volume(t, VOL_YK), host_get_volume(t, _lib.VOL_RECON_OLD),
                    host_get_sino(t, SINO_G)))
    d, h = res
    assert d[0] == h[0] and d[1] == h[1] and d[0] > 0
    for a, c in zip(d[2:], h[2:]):
        same(a, c)


class _DLPackOnly:
    """an array of another library as far as TomoGPU can tell: nothing but the DLPack protocol and a shape"""

    def __init__(self, t):
        self._t, self.shape = t, tuple(t.shape)

    def __dlpack__(self, **kw):
        return self._t.__dlpack__(**kw)

    def __dlpack_device__(self):
        return self._t.__dlpack_device__()


def test_tomogpu_takes_and_returns_device_tensors(gpu):
    nx, n, P = 33, 16, 5
    ang = np.linspace(-60.0, 60.0, P)
    b = np.abs(values32((nx, n, P), 100)) * 1e-2
    ref = TomoGPU(ang, b, gpu_id=0)
    ref.sirt(3)
    want = ref.get_recon()
    assert want.dtype == np.float64 and want.any()
    same(ref.get_projections(), b)
    for given in (torch.from_numpy(b).to(DEV), _DLPackOnly(torch.from_numpy(b).to(DEV)), torch.from_numpy(b.astype(np.float64)).to(DEV),
                  torch.from_numpy(np.ascontiguousarray(b.transpose(0, 2, 1))).to(DEV).transpose(1, 2)):
        tg = TomoGPU(ang, given)                               # no gpu_id: the tensor's device
        assert tg.tomo.gpuID == 0 and tg.tomo.get_option("stage_bytes") == 0
        tg.sirt(3)
        same(tg.get_recon(), want)
        r = tg.get_recon(as_tensor=True)
        assert r.device == DEV and r.dtype == torch.float32
        same(r.cpu().numpy().astype(np.float64), want)
        same(tg.get_recon(as_tensor=True, dtype=torch.float64), want)
        p = tg.get_projections(as_tensor=True)
        assert p.device == DEV and p.dtype == torch.float32
        same(p, b)
        same(tg.get_projections(), b)
    tg.set_tilt_series(torch.from_numpy(2 * b).to(DEV))
    same(tg.get_projections(), 2 * b)


@pytest.mark.parametrize("shape", [(33, 16, 5), (130, 32, 7)], ids=["33x16x5", "130x32x7"])
def test_sub_slab_group_takes_its_rows_by_view(gpu, shape):
    nx, n, P = shape
    t = tomoengine(nx, n, angles(P), device=0, sub_slabs=2)
    a64, want = values64((nx, n, n), 110)
    b = values32((nx, n, P), 111)
    t.set_volume_tensor(torch.from_numpy(a64).to(DEV), VOL_ORIGINAL)
    t.set_tilt_series_tensor(torch.from_numpy(b).to(DEV), SINO_PUBLIC)
    same(t.get_volume(VOL_ORIGINAL), want)                                       # the host path reads what the tensors wrote
    same(t.get_projections(), pytvlib.pack_tilt_series(b))
    h = values32((nx, n, n), 112)
    t.set_volume(h, VOL_RECON)                                                   # ... and the tensors read what the host path wrote
    same(t.get_volume_tensor(VOL_RECON), h)
    same(t.get_volume_tensor(VOL_RECON, dtype=torch.float64), h.astype(np.float64))
    same(t.get_projections_tensor(SINO_B, SINO_PUBLIC), b)
    same(t.get_projections_tensor(SINO_B, SINO_PACKED), pytvlib.pack_tilt_series(b))
    assert t.get_option("stage_bytes") > 0                                       # (the host calls above; the tensor calls: next test)


def test_slab_engines_take_their_rows_of_one_global_tensor(gpu):
    """Two slab engines on one device (the product's thread world): each takes rows [first, first + nloc) of ONE global tensor and the
    local getters hand those rows back.  These engines run on torch's stream: the path without events."""
    nx, n, P = 65, 16, 5
    x, b = values32((nx, n, n), 120), values32((nx, n, P), 121)
    xt, bt = torch.from_numpy(x).to(DEV), torch.from_numpy(b).to(DEV)
    torch.cuda.synchronize(DEV)

    def body(comm):
        t = tomoengine(nx, n, angles(P), device=0, comm=comm)
        first, nloc = slab_partition(nx, 2, comm.rank)
        assert (t.first, t.nloc) == (first, nloc)
        t.set_volume_tensor(xt, VOL_RECON)
        t.set_tilt_series_tensor(bt, SINO_PUBLIC)
        vol, sino = t.get_volume_tensor(VOL_RECON), t.get_projections_tensor(SINO_B, SINO_PUBLIC, dtype=torch.float64)
        assert t.get_option("stage_bytes") == 0
        return (first, nloc, vol.cpu().numpy(), sino.cpu().numpy(), host_get_volume(t, VOL_RECON), host_get_sino(t, SINO_B), t.get_volume(VOL_RECON))
    res = ThreadRing(2).run(body)
    assert [r[1] for r in res] == [33, 32]
    for first, nloc, vol, sino, hvol, hsino, whole in res:
        same(vol, x[first:first + nloc])
        same(sino, b[first:first + nloc].astype(np.float64))
        same(hvol, x[first:first + nloc])
        same(hsino, pytvlib.pack_tilt_series(b[first:first + nloc]))
        same(whole, x)                                                           # the gathering getter is unchanged
