"""Grouped 3x3 convolution (csrc/conv_grouped.hip), element by element.

Integer operands make the reference exact. x and dy are integers in [-3, 3]
and w integers in [-2, 2], so every product and every partial sum of all three
passes is an integer far below 2^24: fp32 accumulation is exact in any order
and for any split count, and the one rounding to the output dtype is
round-to-nearest-even of an exactly known value. The kernels' results must
therefore equal `ref.to(dt)`, where `ref` is torch's fp32 conv ON THE CPU with
`groups`, under `torch.equal`: no tolerance anywhere in sections a to e. A
failure reports how many elements differ and the first few indices with their
pack (c // P) and tile (h // TH, w // 16), which points at the addressing
term that is wrong.

EXACT_SHAPES reaches every kernel variant on a tile other than the first;
`grouped_dispatch` mirrors the host dispatch in plain Python, and
tests/test_conv_grouped_cpu.py checks the list against it without a GPU.

The only tolerance in this file is test_conv_grouped_gpu.py's TOL, in the
module-level routing test (section g), which runs on random data.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from mi355x_ddp.ops import conv as convmod
from mi355x_ddp.ops.conv import MI355Conv2d, MIOPEN, grouped_calls

pytestmark = pytest.mark.gpu

DEV = "cuda"
CL = torch.channels_last
DTYPES = [torch.bfloat16, torch.float16]
# relative Frobenius error, the values of tests/test_conv_grouped_gpu.py;
# used by section g only
TOL = {torch.float16: 5e-4, torch.bfloat16: 4e-3}
TW, WTH = 16, 8

# (N, C, H, W, groups, stride)
EXACT_SHAPES = [
    (2, 32, 18, 35, 8, 2),    # P32 s2: fwd 2x2 tiles, ZINS dgrad 3x3 with odd
                              # tile origins, wgrad S2 on 8 tiles
    (2, 64, 17, 34, 4, 1),    # Cg 16, two packs, 3x3 tiles, ragged last ones
    (2, 128, 18, 35, 2, 2),   # P64 s2: TH = 4 fwd 3x2 tiles, P64 ZINS 3x3,
                              # P64 S2 wgrad 2x2; two packs, two images
    (1, 128, 9, 18, 2, 1),    # P64 s1, 2x2 tiles
    (3, 64, 9, 17, 2, 2),     # Cg 32, three images, odd extents
    (2, 32, 1, 1, 8, 1),      # degenerate extents: ambiguous channels_last
    (2, 32, 2, 2, 8, 2),      # strides, patches that are mostly padding
    (1, 32, 1, 40, 8, 2),
    (1, 32, 40, 1, 8, 1),
]
SPLIT_SHAPES = [(3, 32, 9, 17, 8, 1), EXACT_SHAPES[2]]
RANGE_SHAPES = [EXACT_SHAPES[0], EXACT_SHAPES[2]]     # one P32, one P64
INF_SHAPE = (1, 64, 8, 8, 8, 1)                       # Cg 8, two packs


def grouped_dispatch(shape):
    """Plain-Python mirror of the host dispatch of csrc/conv_grouped.hip: per
    pass the kernel instantiation a shape launches, the tile height and the
    extents its tiles cover. fwd / dgrad variants are (P, S, TH, ZINS), wgrad
    variants (P, S)."""
    N, C, H, W, groups, stride = shape
    P = max(C // groups, 32)
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    fwd_th = 4 if (P, stride) == (64, 2) else 8

    def one(variant, th, eh, ew):
        return dict(variant=variant, TH=th, extent=(eh, ew),
                    tiles_h=-(-eh // th), tiles_w=-(-ew // TW),
                    packs=C // P, N=N)

    return {"fwd": one((P, stride, fwd_th, False), fwd_th, OH, OW),
            "dgrad": one((P, 1, 8, stride == 2), 8, H, W),
            "wgrad": one((P, stride), WTH, OH, OW)}


def _ids(v):
    if isinstance(v, torch.dtype):
        return str(v).replace("torch.", "")
    if isinstance(v, tuple):
        return "x".join(str(i) for i in v)
    return None


def _C():
    from mi355x_ddp import _C
    return _C


def _dev(t):
    return t.to(DEV).contiguous(memory_format=CL)


class _Case:
    """Integer operands and the exact fp32 CPU reference of all three passes.
    Built once per shape and never written to."""

    def __init__(self, shape):
        N, C, H, W, groups, stride = shape
        Cg = C // groups
        g = torch.Generator().manual_seed(977 + sum(shape))
        self.x = torch.randint(-3, 4, (N, C, H, W), generator=g).float()
        self.w = torch.randint(-2, 3, (C, Cg, 3, 3), generator=g).float()
        xr = self.x.clone().requires_grad_(True)
        wr = self.w.clone().requires_grad_(True)
        y = F.conv2d(xr, wr, None, stride, 1, 1, groups)
        self.dy = torch.randint(-3, 4, y.shape, generator=g).float()
        self.dx, self.dw = torch.autograd.grad(y, (xr, wr), self.dy)
        self.y = y.detach()
        for t in (self.y, self.dx, self.dw):
            assert t.abs().max() < 2 ** 24 and (t != 0).any()
        self.shape, self.P = shape, max(Cg, 32)
        self.H, self.W, self.groups, self.stride = H, W, groups, stride
        self.disp = grouped_dispatch(shape)


@functools.lru_cache(maxsize=None)
def _case(shape):
    return _Case(shape)


def _assert_exact(name, got, want, P, TH=None):
    """got (a device tensor) equals want (CPU, same dtype) element by element;
    TH is the pass's tile height, None for the filter gradient."""
    assert got.dtype == want.dtype and got.shape == want.shape, \
        (name, got.dtype, tuple(got.shape), want.dtype, tuple(want.shape))
    assert got.is_contiguous(memory_format=CL), name
    got = got.cpu()
    if torch.equal(got, want):
        return
    bad = (got != want).nonzero()     # a NaN differs from everything
    lines = []
    for n, c, h, w in bad[:8].tolist():
        where = f"pack {c // P}, tile ({h // TH}, {w // TW})" if TH else \
            f"pack {n // P}"
        lines.append(f"  ({n}, {c}, {h}, {w}) {where}: got "
                     f"{got[n, c, h, w].item()} want {want[n, c, h, w].item()}")
    raise AssertionError(
        f"{name}: {len(bad)} of {want.numel()} elements differ; first "
        f"(n, c, h, w):\n" + "\n".join(lines))


# ---- a. three passes, exact, every variant off the first tile ---------------

@pytest.mark.parametrize("dt", DTYPES, ids=_ids)
@pytest.mark.parametrize("shape", EXACT_SHAPES, ids=_ids)
def test_three_passes_exact(shape, dt):
    c = _case(shape)
    x, w, dy = _dev(c.x.to(dt)), _dev(c.w.to(dt)), _dev(c.dy.to(dt))
    wp, wpT = _C().conv_grouped_prep(w, c.groups)
    y = _C().conv_grouped_fwd(x, wp, c.stride)
    dx = _C().conv_grouped_dgrad(dy, wpT, c.H, c.W, c.stride)
    dw = _C().conv_grouped_wgrad(dy, x, c.groups, c.stride, 0)
    _assert_exact("y", y, c.y.to(dt), c.P, c.disp["fwd"]["TH"])
    _assert_exact("dx", dx, c.dx.to(dt), c.P, c.disp["dgrad"]["TH"])
    _assert_exact("dw", dw, c.dw.to(dt), c.P)


# ---- b. wgrad split ranges ---------------------------------------------------

@pytest.mark.parametrize("dt", DTYPES, ids=_ids)
@pytest.mark.parametrize("shape", SPLIT_SHAPES, ids=_ids)
def test_wgrad_splits_exact(shape, dt):
    """5 and 7 put split boundaries inside an image, tiles + 5 is clamped to
    one split per tile. Every split count gives the reference, so all agree."""
    c = _case(shape)
    d = c.disp["wgrad"]
    tiles = d["N"] * d["tiles_h"] * d["tiles_w"]
    assert tiles > 7
    x, dy = _dev(c.x.to(dt)), _dev(c.dy.to(dt))
    want = c.dw.to(dt)
    for splits in (1, 2, 5, 7, tiles, tiles + 5, 0):
        dw = _C().conv_grouped_wgrad(dy, x, c.groups, c.stride, splits)
        _assert_exact(f"dw splits={splits}", dw, want, c.P)


# ---- c. conv_grouped_prep against its documented layout ----------------------

def _packed_by_definition(w, Cg):
    """wf[pack][i*3+j][k][c] = w[pack*P + k][c % Cg][i][j] and
    wb[pack][i*3+j][c][k] = w[pack*P + k][c % Cg][2-i][2-j] for k, c of one
    group, else 0 (the header comment of grouped_prep_kernel), on int16 bits."""
    C = w.shape[0]
    P = max(Cg, 32)
    wf = torch.zeros(C // P, 9, P, P, dtype=w.dtype)
    wb = torch.zeros(C // P, 9, P, P, dtype=w.dtype)
    for pack in range(C // P):
        for k in range(P):
            lo = (k // Cg) * Cg           # first channel of k's group
            for i in range(3):
                for j in range(3):
                    row = w[pack * P + k, :, i, j]
                    wf[pack, i * 3 + j, k, lo:lo + Cg] = row
                    wb[pack, (2 - i) * 3 + (2 - j), lo:lo + Cg, k] = row
    return wf, wb


@pytest.mark.parametrize("dt", DTYPES, ids=_ids)
@pytest.mark.parametrize("Cg", [4, 8, 16, 32, 64])
def test_prep_layout_and_strides(Cg, dt):
    """Random 16-bit patterns (NaNs and infinities included, so the compare is
    on the bits), the same filter values through three stridings."""
    C = 128 if Cg == 64 else 64
    g = torch.Generator().manual_seed(31 + Cg)
    big = torch.randint(-32768, 32768, (C, Cg, 5, 5), generator=g,
                        dtype=torch.int16)
    bits = big[:, :, 1:4, 1:4].contiguous()
    wf, wb = _packed_by_definition(bits, Cg)
    # off-diagonal blocks exist and the expectation has them zero
    if Cg < 32:
        assert (wf[:, :, :Cg, Cg:2 * Cg] == 0).all()
    stridings = {
        "channels_last": bits.to(DEV).contiguous(memory_format=CL),
        "nchw": bits.to(DEV),
        "view": big.to(DEV)[:, :, 1:4, 1:4],
    }
    assert not stridings["view"].is_contiguous()
    for name, wbits in stridings.items():
        w = wbits.view(dt)
        assert w.stride() == wbits.stride()
        # prep's output comes from at::empty: leave a freed block of its size
        # full of ones to the allocator, so that zeros it fails to write show
        poison = torch.full((2 * wf.numel(),), -1, dtype=torch.int16,
                            device=DEV)
        del poison
        wp, wpT = _C().conv_grouped_prep(w, C // Cg)
        for what, got, want in (("wp", wp, wf), ("wpT", wpT, wb)):
            assert got.dtype == dt and got.shape == want.shape, (name, what)
            assert got.is_contiguous(), (name, what)
            gb = got.view(torch.int16).cpu()
            bad = (gb != want).nonzero()
            assert len(bad) == 0, (
                f"{what} from the {name} filter: {len(bad)} of "
                f"{want.numel()} differ; first (pack, tap, row, col): "
                f"{bad[:8].tolist()}")


# ---- d. fp16 range -----------------------------------------------------------

@pytest.mark.parametrize("shape", RANGE_SHAPES, ids=_ids)
def test_fp16_overflow_is_inf_everywhere(shape):
    """x = w = dy = 256: even a corner output sums 65536 over at least one
    tap and four channels, above fp16's 65504. Every element of y, dx and dw
    is +inf: no saturation to 65504, no NaN."""
    N, C, H, W, groups, stride = shape
    h = torch.float16
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    x = torch.full((N, C, H, W), 256.0, dtype=h, device=DEV).contiguous(
        memory_format=CL)
    w = torch.full((C, C // groups, 3, 3), 256.0, dtype=h,
                   device=DEV).contiguous(memory_format=CL)
    dy = torch.full((N, C, OH, OW), 256.0, dtype=h, device=DEV).contiguous(
        memory_format=CL)
    wp, wpT = _C().conv_grouped_prep(w, groups)
    y = _C().conv_grouped_fwd(x, wp, stride)
    dx = _C().conv_grouped_dgrad(dy, wpT, H, W, stride)
    dw = _C().conv_grouped_wgrad(dy, x, groups, stride, 0)
    for name, got, shp in (("y", y, dy.shape), ("dx", dx, x.shape),
                           ("dw", dw, w.shape)):
        assert got.shape == shp and got.dtype == h, name
        n_bad = int((~torch.isposinf(got)).sum())
        assert n_bad == 0, f"{name}: {n_bad} of {got.numel()} are not +inf"


@pytest.mark.parametrize("shape", RANGE_SHAPES, ids=_ids)
def test_fp16_subnormal_operands_and_results(shape):
    """The integer case with x (forward) or dy (dgrad, wgrad) scaled by 2^-24:
    that operand is fp16-subnormal throughout and every result is an integer
    multiple of 2^-24 below 2^-14, a subnormal fp16 that is exactly known."""
    c = _case(shape)
    h, lsb = torch.float16, 2.0 ** -24
    for ref in (c.y, c.dx, c.dw):
        assert ref.abs().max() <= 1023    # fits fp16's subnormal range

    def tiny(t):
        s = (t * lsb).to(h)
        assert torch.equal(s.float(), t * lsb)
        assert (s.abs().float() < 2.0 ** -14).all() and (s != 0).any()
        return _dev(s)

    def expected(ref):
        e = (ref * lsb).to(h)
        assert (e != 0).any() and torch.equal(e.float(), ref * lsb)
        return e

    x, w = _dev(c.x.to(h)), _dev(c.w.to(h))
    wp, wpT = _C().conv_grouped_prep(w, c.groups)
    y = _C().conv_grouped_fwd(tiny(c.x), wp, c.stride)
    dx = _C().conv_grouped_dgrad(tiny(c.dy), wpT, c.H, c.W, c.stride)
    dw = _C().conv_grouped_wgrad(tiny(c.dy), x, c.groups, c.stride, 0)
    _assert_exact("y", y, expected(c.y), c.P, c.disp["fwd"]["TH"])
    _assert_exact("dx", dx, expected(c.dx), c.P, c.disp["dgrad"]["TH"])
    _assert_exact("dw", dw, expected(c.dw), c.P)


# ---- e. non-finite values ----------------------------------------------------

@pytest.mark.parametrize("dt", DTYPES, ids=_ids)
def test_inf_is_kept_and_stays_in_its_pack(dt):
    """One +inf in dy (in x for the forward) at channel k0 of pack 0. It must
    reach everything that depends on it (the fp16 loss scaler relies on that)
    and nothing of pack 1. The other groups of pack 0 are not looked at: the
    block-diagonal filter multiplies their zeros by the inf (NOTES.md)."""
    c = _case(INF_SHAPE)
    N, C, H, W, groups, stride = INF_SHAPE
    Cg, P = C // groups, c.P
    k0, ph, pw = 13, 3, 4                 # group 1 of pack 0, interior pixel
    grp = slice((k0 // Cg) * Cg, (k0 // Cg + 1) * Cg)
    nb = (slice(None), grp, slice(ph - 1, ph + 2), slice(pw - 1, pw + 2))
    x, w, dy = _dev(c.x.to(dt)), _dev(c.w.to(dt)), _dev(c.dy.to(dt))
    wp, wpT = _C().conv_grouped_prep(w, groups)

    dy_inf = c.dy.to(dt)
    dy_inf[0, k0, ph, pw] = float("inf")
    dy_inf = _dev(dy_inf)
    dw = _C().conv_grouped_wgrad(dy_inf, x, groups, stride, 0).cpu()
    dx = _C().conv_grouped_dgrad(dy_inf, wpT, H, W, stride).cpu()
    assert not torch.isfinite(dw[k0]).any(), \
        f"dw[{k0}]: {int(torch.isfinite(dw[k0]).sum())} of {9 * Cg} finite"
    assert not torch.isfinite(dx[nb]).any(), \
        f"dx: {int(torch.isfinite(dx[nb]).sum())} of {9 * Cg} finite"
    assert torch.equal(dw[P:], c.dw[P:].to(dt)), "dw pack 1"
    assert torch.equal(dx[:, P:], c.dx[:, P:].to(dt)), "dx pack 1"

    x_inf = c.x.to(dt)
    x_inf[0, k0, ph, pw] = float("inf")
    y = _C().conv_grouped_fwd(_dev(x_inf), wp, stride).cpu()
    assert not torch.isfinite(y[nb]).any(), \
        f"y: {int(torch.isfinite(y[nb]).sum())} of {9 * Cg} finite"
    assert torch.equal(y[:, P:], c.y[:, P:].to(dt)), "y pack 1"


# ---- f. the host checks refuse bad calls before any launch -------------------

def _act(C=32, H=8, W=8, dt=torch.bfloat16, N=1):
    return torch.zeros(N, C, H, W, dtype=dt, device=DEV).contiguous(
        memory_format=CL)


def _filt(C, Cg, dt=torch.bfloat16):
    return torch.zeros(C, Cg, 3, 3, dtype=dt, device=DEV).contiguous(
        memory_format=CL)


@pytest.mark.parametrize("C, Cg, msg", [
    (32, 2, "channels per group"), (128, 128, "channels per group"),
    (16, 4, "multiple of 32")])
def test_refused_group_widths(C, Cg, msg):
    with pytest.raises(RuntimeError, match=msg):
        _C().conv_grouped_prep(_filt(C, Cg), C // Cg)
    with pytest.raises(RuntimeError, match=msg):
        _C().conv_grouped_wgrad(_act(C), _act(C), C // Cg, 1, 0)


def test_refused_prep_filter_shape():
    with pytest.raises(RuntimeError, match="but groups is 8"):
        _C().conv_grouped_prep(_filt(32, 8), 8)      # w.size(1) != C / groups


def test_refused_fwd_calls():
    C = _C()
    wp = C.conv_grouped_prep(_filt(32, 4), 8)[0]
    with pytest.raises(RuntimeError, match="stride must be 1 or 2"):
        C.conv_grouped_fwd(_act(), wp, 3)
    with pytest.raises(RuntimeError, match="bf16 or fp16"):
        C.conv_grouped_fwd(_act(dt=torch.float32), wp, 1)
    nchw = torch.zeros(1, 32, 8, 8, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match="channels_last"):
        C.conv_grouped_fwd(nchw, wp, 1)
    with pytest.raises(RuntimeError, match="share one dtype"):
        C.conv_grouped_fwd(_act(dt=torch.float16), wp, 1)
    with pytest.raises(RuntimeError, match="packed filter"):
        C.conv_grouped_fwd(_act(C=64), wp, 1)        # wp packed for C = 32
    wide = C.conv_grouped_prep(_filt(128, 4), 32)[0]
    sliced = wide[::2]                               # [2][9][32][32], strided
    assert sliced.shape[0] * 32 == 64 and not sliced.is_contiguous()
    with pytest.raises(RuntimeError, match="packed filter"):
        C.conv_grouped_fwd(_act(C=64), sliced, 1)
    with pytest.raises(RuntimeError, match="batch must be in"):
        C.conv_grouped_fwd(_act(N=0), wp, 1)


def test_refused_backward_calls():
    C = _C()
    wpT = C.conv_grouped_prep(_filt(32, 4), 8)[1]
    dy = _act(H=4, W=4)
    with pytest.raises(RuntimeError, match="stride must be 1 or 2"):
        C.conv_grouped_dgrad(dy, wpT, 10, 10, 3)
    with pytest.raises(RuntimeError, match="stride must be 1 or 2"):
        C.conv_grouped_wgrad(dy, _act(H=10, W=10), 8, 3, 0)
    # a 9 x 8 input at stride 2 has a 5 x 4 output, not 4 x 4
    with pytest.raises(RuntimeError, match="extents do not belong"):
        C.conv_grouped_dgrad(dy, wpT, 9, 8, 2)
    with pytest.raises(RuntimeError, match="does not belong to x"):
        C.conv_grouped_wgrad(dy, _act(H=9, W=8), 8, 2, 0)
    with pytest.raises(RuntimeError, match="share one dtype"):
        C.conv_grouped_wgrad(dy, _act(H=8, W=8, dt=torch.float16), 8, 2, 0)
    with pytest.raises(RuntimeError, match="splits must be >= 0"):
        C.conv_grouped_wgrad(dy, _act(H=8, W=8), 8, 2, -1)
    with pytest.raises(RuntimeError, match="batch must be in"):
        C.conv_grouped_dgrad(_act(H=4, W=4, N=0), wpT, 8, 8, 2)
    with pytest.raises(RuntimeError, match="batch must be in"):
        C.conv_grouped_wgrad(_act(H=4, W=4, N=0), _act(N=0), 8, 2, 0)


# ---- g. routing with the tuner on --------------------------------------------

def _module_step(dt, stride):
    """One forward and backward of a (2, 64, 12, 12) groups-8 module under
    autocast; the fp32 CPU module on the same rounded operands, as
    test_conv_grouped_gpu.test_module_under_bf16_autocast computes it."""
    torch.manual_seed(3)
    ref = torch.nn.Conv2d(64, 64, 3, stride=stride, padding=1, groups=8,
                          bias=False)
    conv = MI355Conv2d(64, 64, 3, stride=stride, padding=1, groups=8,
                       bias=False)
    conv.load_state_dict(ref.state_dict())
    conv = conv.to(DEV).to(memory_format=CL)
    x = torch.randn(2, 64, 12, 12)
    dy = torch.randn(2, 64, 12 // stride, 12 // stride)
    xd = _dev(x).requires_grad_(True)
    grouped_calls.reset()
    with torch.autocast("cuda", dtype=dt):
        y = conv(xd)
    after_fwd = getattr(y.grad_fn, "wpT", None)
    y.backward(_dev(dy.to(dt)))
    after_bwd = getattr(y.grad_fn, "wpT", None)
    with torch.no_grad():
        ref.weight.copy_(ref.weight.to(dt).float())
    xr = x.to(dt).float().requires_grad_(True)
    yr = ref(xr)
    yr.backward(dy.to(dt).float())

    def rel(got, want):
        got = got.float().cpu()
        return ((got - want).norm() / want.norm()).item()

    assert y.dtype == dt and conv.weight.grad.dtype == torch.float32
    errs = (rel(y, yr.detach()), rel(xd.grad, xr.grad),
            rel(conv.weight.grad, ref.weight.grad))
    return errs, after_fwd, after_bwd


@pytest.mark.parametrize("dt, stride", [
    (torch.bfloat16, 1), (torch.bfloat16, 2), (torch.float16, 1)], ids=_ids)
def test_module_routing_with_the_tuner_on(monkeypatch, dt, stride):
    monkeypatch.setenv("MI355X_AUTOTUNE", "1")
    monkeypatch.setenv("MI355X_NATIVE_GROUPED", "1")
    # the process-wide cache goes back to what it was
    monkeypatch.setattr(convmod, "_TUNE_CACHE", {})
    errs, _, _ = _module_step(dt, stride)
    print(f"tuned {dt} stride {stride}: y/dx/dw rel err",
          ["%.3e" % e for e in errs], "\n" + convmod.tune_report())
    assert max(errs) < TOL[dt], errs
    cache = convmod._TUNE_CACHE
    keys = {kind: [k for k in cache if k[0] == kind]
            for kind in ("g_fwd", "g_dgrad", "g_wgrad")}
    assert all(len(v) == 1 for v in keys.values()) and len(cache) == 3, cache
    kf, kd, kw = (keys[k][0] for k in ("g_fwd", "g_dgrad", "g_wgrad"))
    assert all(k[1] == dt for k in (kf, kd, kw))
    assert cache[kf] in (0, MIOPEN) and cache[kd] in (0, MIOPEN)
    assert cache[kw] in tuple(
        ("splits", s) for s in convmod._GROUPED_WGRAD_SPLITS) + (MIOPEN,)
    native = tuple(int(cache[k] != MIOPEN) for k in (kf, kd, kw))
    assert (grouped_calls.fwd, grouped_calls.dgrad, grouped_calls.wgrad) == \
        native
    report = convmod.tune_report().splitlines()
    assert len(report) == 3
    for key in (kf, kd, kw):
        line = [ln for ln in report if ln.split()[0] == key[0]]
        assert len(line) == 1
        choice = cache[key]
        if choice == MIOPEN:
            label = "MIOpen"
        elif key[0] == "g_wgrad":
            label = "native grouped, splits " + \
                ("auto" if choice[1] == 0 else str(choice[1]))
        else:
            label = "native grouped"
        assert line[0].endswith("-> " + label), (line, label)

    # the forward on MIOpen, the backward native: backward packs wpT itself
    cache[kf], cache[kd], cache[kw] = MIOPEN, 0, ("splits", 1)
    errs, after_fwd, after_bwd = _module_step(dt, stride)
    print(f"MIOpen fwd, native bwd {dt} stride {stride}: y/dx/dw rel err",
          ["%.3e" % e for e in errs])
    assert (grouped_calls.fwd, grouped_calls.dgrad, grouped_calls.wgrad) == \
        (0, 1, 1)
    assert after_fwd is None and after_bwd is not None
    assert after_bwd.shape == (2, 9, 32, 32) and after_bwd.dtype == dt
    assert max(errs) < TOL[dt], errs
    assert len(cache) == 3
