"""Dense implicit-GEMM convolution (csrc/conv_igemm.hip), element by element.

Integer operands make the reference exact. x and dy are integers in [-3, 3]
and w integers in [-2, 2] (a wide set: both in [-15, 15]), so every product
and every partial sum of all three passes is an integer far below 2^24: fp32
accumulation is exact in any order, for any tile, any split count and any
interleaving of atomic adds, and the one rounding to the output dtype is
round-to-nearest-even of an exactly known value. Every kernel variant has one
legal output, `ref.to(dt)`, where `ref` is torch's fp32 conv ON THE CPU, and
it is compared under `torch.equal`: there is no tolerance in this file. A
failure reports how many elements differ and the first few indices with their
GEMM tile (M tile, N tile, for the tile sizes launched) and whether the pixel
lies on an image border, which points at the addressing term that is wrong.

Every shape but the 1x1 image and the one large weight-grad case has
H != W, so a swap of the two extents anywhere (decode_m,
decode_m2, tap_coord's limits, the v2 weight-grad's row offsets, the host's
ConvDims) moves elements. `igemm_dispatch` and `wgrad_dispatch` mirror the
host dispatch in plain Python; `launched_igemm` and `launched_wgrad` list what
the sections below launch, from the same constants the tests loop over, and
tests/test_conv_exact_cpu.py checks without a GPU that the lists still reach
every instantiation the host can launch.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from mi355x_ddp.ops import conv as convmod
from mi355x_ddp.ops.conv import rotate_wT

pytestmark = pytest.mark.gpu

DEV = "cuda"
CL = torch.channels_last
DTYPES = [torch.bfloat16, torch.float16]
BK = 64
CUS = 256            # CU count of the MI355X, for the reduce variant

# (N, C, H, W, K, R, stride, pad)
FAST_SHAPE = (2, 64, 9, 14, 64, 3, 1, 1)
PARITY_SHAPE = (3, 64, 10, 14, 128, 3, 2, 1)
ODD_S2_SHAPE = (3, 64, 9, 13, 128, 3, 2, 1)
S2_1X1_SHAPE = (2, 64, 8, 12, 128, 1, 2, 0)
STEM_SHAPE = (2, 3, 10, 13, 64, 3, 1, 1)
STEM_7X7_SHAPE = (2, 3, 16, 22, 64, 7, 2, 3)
LIN128_SHAPE = (2, 128, 8, 12, 256, 1, 1, 0)
LIN256_SHAPE = (2, 64, 16, 20, 256, 1, 1, 0)
N100_SHAPE = (2, 64, 8, 12, 100, 3, 1, 1)
GENERIC_SHAPE = (2, 24, 9, 7, 40, 3, 1, 1)
GENERIC_1X1_SHAPE = (2, 160, 5, 7, 100, 1, 1, 0)
S3_5X5_SHAPE = (2, 64, 11, 14, 64, 5, 3, 2)
EXACT_SHAPES = [
    FAST_SHAPE,                       # FAST; M = 252: ragged on 64 and 128
    PARITY_SHAPE,                     # parity dgrad, 4 classes, class M = 105;
                                      # forward N = 128 on the 228 tile
    ODD_S2_SHAPE,                     # stride 2, odd extents: MODE 1, t % 2
    S2_1X1_SHAPE,                     # 1x1 s2: memset + one class, the zeros
    STEM_SHAPE,                       # PADC stem on the 64 and 128 tile
    STEM_7X7_SHAPE,                   # 7x7 PADC stem, reduction 196 -> 256
    LIN128_SHAPE,                     # 128-wide N tile; LIN 128x128 wgrad
    LIN256_SHAPE,                     # LIN 256x64 wgrad; forward M = 640
    (2, 256, 4, 6, 512, 3, 1, 1),     # 36 reduction tiles on M = 48: split-K
                                      # fwd / dgrad; v2 128x128 wgrad 4 x 18
    (3, 256, 8, 9, 256, 3, 1, 1),     # split-K, ragged 2nd M tile, 2 N tiles
    N100_SHAPE,                       # FAST fwd N = 100: ragged 128 tile, the
                                      # N % 8 != 0 stores of the split reduce;
                                      # generic dgrad; wgrad off FAST (K % 16)
    GENERIC_SHAPE,                    # generic in all passes, ragged M, N, K
    GENERIC_1X1_SHAPE,                # the same, 1x1
    (1, 1, 6, 9, 16, 3, 1, 1),        # tiny channel counts, not the stem's
    (2, 4, 6, 9, 16, 3, 1, 1),
    (2, 64, 9, 11, 64, 3, 1, 0),      # off the ResNet menu: 3x3 pad 0,
    (2, 64, 7, 10, 64, 1, 1, 1),      # 1x1 pad 1 (border outputs all padding),
    S3_5X5_SHAPE,                     # 5x5 stride 3,
    (5, 64, 10, 12, 64, 3, 2, 0),     # stride 2 pad 0: parity with P < H / 2
    (1, 64, 1, 5, 64, 3, 1, 1),       # degenerate extents
    (2, 64, 1, 1, 128, 1, 1, 0),      # ambiguous channels_last strides
]
# tile 228 with splits > 1 is a split-K launch in the forward of all three
# and in the input-grad of the first two (the third's is generic: K = 100)
SPLITK_SHAPES = [EXACT_SHAPES[8], EXACT_SHAPES[9], N100_SHAPE]
SPLITK_SPLITS = (2, 3, 5, 1000)       # and one past the reduction-tile count
TILES = (64, 128, 228)

# section c: on the first two the 128-row and the 256-row tiles each have a
# ragged second M tile; N = 576 and N = 64 are ragged on the 128-wide tile
WGRAD_SHAPES = [
    (2, 64, 9, 14, 320, 3, 1, 1),     # M = 320, N = 576
    (2, 64, 8, 12, 320, 1, 1, 0),     # M = 320, N = 64, LIN
    LIN128_SHAPE, LIN256_SHAPE,
    GENERIC_SHAPE,                    # every wtile falls back to v1 generic
    N100_SHAPE,                       # the same through K % 16 != 0
    STEM_SHAPE,                       # every wtile falls back to v1 PADC
    STEM_7X7_SHAPE,                   # the same on two N tiles (196 columns)
]
WTILES = (1, 2, 3, 4, 5, 6, 8, 9)
WSPLITS = (1, 2, 3, -1, 0, 128, 1000)
# the one large case: 128 reduction chunks, which the wide z-group reduces
# (ZW 8 and 16) need; only the pairs that use them
WGRAD_BIG_SHAPE = (8, 64, 32, 32, 64, 3, 1, 1)
WGRAD_BIG_PAIRS = ((1, 128), (1, 1000), (2, 128), (3, 128), (8, 1000),
                   (9, 128), (4, 128), (1, -1), (1, 0))

# wide operands, integers in [-15, 15]: one FAST and one generic shape whose
# three reductions (R*S*C, R*S*K, N*P*Q) are long enough for a tenth of every
# result to pass 2048, where neither 16-bit format holds every integer
WIDE_SHAPES = [(4, 64, 10, 12, 64, 3, 1, 1), (4, 72, 9, 12, 72, 3, 1, 1)]

# section d: FAST, generic, stem and split-K (ragged N = 100)
BN_SHAPES = [FAST_SHAPE, GENERIC_1X1_SHAPE, STEM_SHAPE, N100_SHAPE]
BN_LAUNCHES = ((0, 1), (64, 1), (128, 1), (228, 1), (228, 3))
BN_SCALES = (1.0, -1.0, 2.0, 0.5, 0.0)

PUBLIC_SHAPES = [FAST_SHAPE, ODD_S2_SHAPE, S3_5X5_SHAPE]      # section e
PIN_SHAPE = EXACT_SHAPES[8]                                   # section f
PIN_IGEMM, PIN_WGRAD = (228, 4), (4, 0)


# ---- the host dispatch of csrc/conv_igemm.hip in plain Python ----------------

def _cdiv(a, b):
    return -(-a // b)


def out_extent(shape):
    N, C, H, W, K, R, stride, pad = shape
    return (H + 2 * pad - R) // stride + 1, (W + 2 * pad - R) // stride + 1


def _pick_bmt(M, N, tile):
    if tile in (64, 128):
        return tile
    return 64 if _cdiv(M, 128) * _cdiv(N, 64) < 384 else 128


def _igemm_splits(M, N, K, splits):
    tiles = _cdiv(M, 128) * _cdiv(N, 128)
    max_ws = max(1, 96 * 1024 * 1024 // (tiles * 128 * 128 * 4))
    return max(1, min(splits, K // BK, max_ws))


def igemm_dispatch(shape, kind, tile=0, splits=1):
    """What conv_fwd_igemm (kind "fwd"), conv_fwd_bn_igemm ("fwd_bn") or
    conv_dgrad_igemm ("dgrad") launches: `inst` is the conv_igemm_kernel
    instantiation (MODE, FAST, BMT, PADC, BNT, SPLITK, BNEPI), `grid` its
    grid, `splits` the clamped slice count, `nclass` the parity class count
    (0 off the parity path), `reduce` the split-K reduce as ("igemm", BNEPI)
    or None, M / N / K the GEMM extents the kernel sees (class-local M on the
    parity path) and `image` the (OH, OW) that M rows decode to."""
    Nb, C, H, W, Kout, R, stride, pad = shape
    P, Q = out_extent(shape)
    bn = kind == "fwd_bn"

    def res(inst, M, N, K, nz=1, nclass=0, image=None):
        mode, fast, bmt, padc, bnt, splitk, _ = inst
        gz = nz if splitk else max(nclass, 1)
        return dict(inst=inst, M=M, N=N, K=K, splits=nz, nclass=nclass,
                    grid=(_cdiv(N, bnt), _cdiv(M, bmt), gz), image=image,
                    reduce=("igemm", bn) if splitk else None)

    if kind in ("fwd", "fwd_bn"):
        M, N, img = Nb * P * Q, Kout, (P, Q)
        if C == 3:
            K = _cdiv(R * R * 4, BK) * BK
            return res((0, False, _pick_bmt(M, N, tile), True, 64, False, bn),
                       M, N, K, image=img)
        K, fast, mode = R * R * C, C % BK == 0, 0
    else:
        assert kind == "dgrad"
        M, N, K, img = Nb * H * W, C, R * R * Kout, (H, W)
        fast, mode = Kout % BK == 0, 1
        if fast and stride == 2 and H % 2 == 0 and W % 2 == 0:
            M2 = Nb * (H // 2) * (W // 2)
            nclass = 1 if (R == 1 and pad == 0) else 4
            t128 = _cdiv(M2, 128) * _cdiv(N, 64) * nclass
            bmt = tile if tile in (64, 128) else (64 if t128 < 384 else 128)
            return res((2, True, bmt, False, 64, False, False), M2, N, K,
                       nclass=nclass, image=img)
    if tile == 228 and fast and N >= 96:
        nz = _igemm_splits(M, N, K, splits)
        if nz > 1:    # the epilogue moves into the reduce
            return res((mode, True, 128, False, 128, True, False), M, N, K,
                       nz=nz, image=img)
        return res((mode, True, 128, False, 128, False, bn), M, N, K,
                   image=img)
    return res((mode, fast, _pick_bmt(M, N, tile), False, 64, False, bn),
               M, N, K, image=img)


def wgrad_dispatch(shape, wtile=0, splits=0, cus=CUS):
    """What conv_wgrad_igemm launches: `tile` is the resolved wtile, `kernel`
    the instantiation as ("v1", FAST, PADC, DIRECT, ATOMIC), ("v2", WGM, WGN,
    DIRECT, CH) or ("lin", WGM, WGN, DIRECT); `path` is "direct", "slab" or
    "atomic"; `reduce` is None (direct), ("rowmajor",) (atomic) or ("frag", ZW,
    V); M / N / K are the GEMM extents (Kout, R*S*Cpad, N*P*Q)."""
    Nb, C, H, W, Kout, R, stride, pad = shape
    P, Q = out_extent(shape)
    stem = C == 3
    cpad = 4 if stem else C
    M, N, K = Kout, R * R * cpad, Nb * P * Q
    fast = C % BK == 0 and Kout % 16 == 0
    lin_ok = fast and not stem and R == 1 and stride == 1 and pad == 0
    tile = wtile
    if tile == 0:
        if lin_ok and M >= 128 and N >= 96:
            tile = 5
        elif lin_ok and M >= 256 and N <= 64:
            tile = 6
        elif fast and not stem and M >= 256 and N <= 64:
            tile = 3
        elif fast and not stem and M >= 128 and N >= 96:
            tile = 2
        else:
            tile = 1
    if tile in (5, 6) and not lin_ok:
        tile -= 3
    if not fast or stem:
        tile = 4 if tile == 4 else 1
    TM = 256 if tile in (3, 6, 9) else 128 if tile in (2, 5, 8) else 64
    TN = 128 if tile in (2, 5, 8) else 64 if tile in (3, 6, 9) else 128
    tm, tn = _cdiv(M, TM), _cdiv(N, TN)
    nchunks = _cdiv(K, BK)
    nzmax = (nchunks + 1) // 2 if tile in (8, 9) else nchunks
    target = cus * (4 if tile in (1, 4) else 2) if splits < 0 else 1024
    nz = splits if splits > 0 else min(target // (tm * tn), nchunks // 8)
    max_ws = 96 * 1024 * 1024 // (tm * tn * TM * TN * 4)
    nz = max(1, min(nz, nzmax, max(max_ws, 1), 1024))
    direct = nz == 1 and not stem and tile != 4
    atomic = not direct and tile == 4
    if tile in (8, 9):
        kernel = ("v2", TM // 64, TN // 64, direct, 2)
    elif tile in (5, 6):
        kernel = ("lin", TM // 64, TN // 64, direct)
    elif tile in (2, 3):
        kernel = ("v2", TM // 64, TN // 64, direct, 1)
    else:
        kernel = ("v1", fast and not stem, stem, direct, atomic)
    reduce = None
    if atomic:
        reduce = ("rowmajor",)
    elif not direct:
        nslots = tm * tn * TM * TN // 4
        seq = splits == 0
        zw = 1
        while not seq and zw < 16 and nslots * zw // 256 < 2 * cus and \
                zw * 8 <= nz:
            zw *= 2
        v = 1 if seq and nslots // 256 < 2 * cus else 4
        reduce = ("frag", 1 if v == 1 else zw, v)
    return dict(tile=tile, TM=TM, TN=TN, grid=(tn, tm, nz), splits=nz,
                kernel=kernel, reduce=reduce, M=M, N=N, K=K,
                path="direct" if direct else "atomic" if atomic else "slab")


def splitk_requests(shape, kind):
    """Section b's split requests for tile 228: the fixed ones and one past
    the pass's reduction-tile count."""
    return SPLITK_SPLITS + (igemm_dispatch(shape, kind)["K"] // BK + 1,)


def launched_igemm():
    """(section, shape, kind, tile, splits) of every forward and input-grad
    launch of sections a, b, d, e and f (each for both dtypes)."""
    out = []
    for shape in EXACT_SHAPES:
        for kind in ("fwd", "dgrad"):
            out.append(("a", shape, kind, 0, 1))
            out += [("b", shape, kind, t, 1) for t in TILES]
            if shape in SPLITK_SHAPES:
                out += [("b", shape, kind, 228, s)
                        for s in splitk_requests(shape, kind)]
    for shape in WIDE_SHAPES:
        out += [("a", shape, kind, 0, 1) for kind in ("fwd", "dgrad")]
    for shape in BN_SHAPES:
        out += [("d", shape, "fwd_bn", t, s) for t, s in BN_LAUNCHES]
    for shape in PUBLIC_SHAPES:
        out += [("e", shape, kind, 0, 1) for kind in ("fwd", "dgrad")]
    out += [("f", PIN_SHAPE, kind) + PIN_IGEMM for kind in ("fwd", "dgrad")]
    return out


def launched_wgrad():
    """(section, shape, wtile, splits) of every weight-grad launch."""
    out = [("a", shape, 0, 0) for shape in EXACT_SHAPES + WIDE_SHAPES]
    for shape in WGRAD_SHAPES:
        out += [("c", shape, t, s) for t in WTILES for s in WSPLITS]
    out += [("c", WGRAD_BIG_SHAPE, t, s) for t, s in WGRAD_BIG_PAIRS]
    out += [("e", shape, 0, 0) for shape in PUBLIC_SHAPES]
    out.append(("f", PIN_SHAPE) + PIN_WGRAD)
    return out


# ---- operands, reference, comparison -----------------------------------------

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
    Built once per (shape, operand range) and never written to. `amax` bounds
    |x| and |dy|, `wmax` bounds |w|."""

    def __init__(self, shape, amax=3, wmax=2):
        N, C, H, W, K, R, stride, pad = shape
        g = torch.Generator().manual_seed(1733 + 7 * amax + sum(shape))
        self.x = torch.randint(-amax, amax + 1, (N, C, H, W),
                               generator=g).float()
        self.w = torch.randint(-wmax, wmax + 1, (K, C, R, R),
                               generator=g).float()
        xr = self.x.clone().requires_grad_(True)
        wr = self.w.clone().requires_grad_(True)
        y = F.conv2d(xr, wr, None, stride, pad)
        assert tuple(y.shape[2:]) == out_extent(shape)
        self.dy = torch.randint(-amax, amax + 1, y.shape, generator=g).float()
        self.dx, self.dw = torch.autograd.grad(y, (xr, wr), self.dy)
        self.y = y.detach()
        for t in (self.y, self.dx, self.dw):
            assert t.abs().max() < 2 ** 24      # fp32 sums are exact
            assert t.abs().max() < 65504        # finite in fp16
            assert (t != 0).any()
        self.shape, self.H, self.W, self.R = shape, H, W, R
        self.stride, self.pad = stride, pad

    def operands(self, dt):
        """x, w, dy and the rotated filter on the device, in dt."""
        w = self.w.to(dt)
        return (_dev(self.x.to(dt)), _dev(w), _dev(self.dy.to(dt)),
                rotate_wT(w.contiguous(memory_format=CL)).to(DEV))


@functools.lru_cache(maxsize=None)
def _case(shape, amax=3, wmax=2):
    return _Case(shape, amax, wmax)


def _where(disp):
    """index -> text: the GEMM tile of an output element of a forward or
    input-grad launch described by `disp`, and its border flag."""
    mode, _, bmt, _, bnt = disp["inst"][:5]
    OH, OW = disp["image"]

    def where(n, c, h, w):
        if mode == 2:       # class-local row of parity class (h % 2, w % 2)
            m = (n * (OH // 2) + h // 2) * (OW // 2) + w // 2
            cls = f"class ({h % 2}, {w % 2}), "
        else:
            m, cls = (n * OH + h) * OW + w, ""
        edge = h in (0, OH - 1) or w in (0, OW - 1)
        return (f"{cls}M tile {m // bmt} of {bmt}, N tile {c // bnt} of "
                f"{bnt}, {'border' if edge else 'interior'} pixel")
    return where


def _assert_exact(name, got, want, where=None, dtype=None):
    """got (a device tensor) equals want (CPU) element by element, in want's
    dtype, shape and channels_last layout."""
    assert got.dtype == (dtype or want.dtype) and got.shape == want.shape, \
        (name, got.dtype, tuple(got.shape), want.dtype, tuple(want.shape))
    assert got.is_contiguous(memory_format=CL), name
    got = got.cpu()
    if torch.equal(got, want):
        return
    bad = (got != want).nonzero()     # a NaN differs from everything
    lines = []
    for idx in bad[:8].tolist():
        n, c, h, w = idx
        lines.append(f"  ({n}, {c}, {h}, {w})"
                     f"{' ' + where(n, c, h, w) if where else ''}: got "
                     f"{got[n, c, h, w].item()} want {want[n, c, h, w].item()}")
    raise AssertionError(
        f"{name}: {len(bad)} of {want.numel()} elements differ; first "
        f"(n, c, h, w):\n" + "\n".join(lines))


def _fwd_dgrad_exact(c, dt, ops, tile, splits=1):
    x, w, dy, wT = ops
    s, p = c.stride, c.pad
    tag = f"tile {tile} splits {splits}"
    y = _C().conv_fwd_igemm(x, w, s, p, tile, splits)
    _assert_exact(f"y {tag}", y, c.y.to(dt),
                  _where(igemm_dispatch(c.shape, "fwd", tile, splits)))
    dx = _C().conv_dgrad_igemm(dy, wT, c.H, c.W, s, p, tile, splits)
    _assert_exact(f"dx {tag}", dx, c.dx.to(dt),
                  _where(igemm_dispatch(c.shape, "dgrad", tile, splits)))


# ---- a. three passes, default launch -----------------------------------------

def _three_passes(c, dt):
    ops = c.operands(dt)
    _fwd_dgrad_exact(c, dt, ops, 0)
    dw = _C().conv_wgrad_igemm(ops[2], ops[0], c.R, c.R, c.stride, c.pad)
    _assert_exact("dw", dw, c.dw.to(dt))


@pytest.mark.parametrize("dt", DTYPES, ids=_ids)
@pytest.mark.parametrize("shape", EXACT_SHAPES, ids=_ids)
def test_three_passes_exact(shape, dt):
    _three_passes(_case(shape), dt)


@pytest.mark.parametrize("dt", DTYPES, ids=_ids)
@pytest.mark.parametrize("shape", WIDE_SHAPES, ids=_ids)
def test_three_passes_exact_wide_operands(shape, dt):
    """Operands in [-15, 15]: a tenth and more of every result lies beyond
    2048 (asserted on the CPU in test_conv_exact_cpu.py), so the kernels' one
    rounding, ties included, is compared with torch's in both formats."""
    _three_passes(_case(shape, 15, 15), dt)


def test_1x1_stride2_dgrad_zeros_are_zeros():
    """The classes the 1x1 stride-2 input-grad never computes are exact
    zeros, on memory that held something else: the output block is first
    handed to the allocator full of ones."""
    c = _case(S2_1X1_SHAPE)
    for dt in DTYPES:
        x, w, dy, wT = c.operands(dt)
        assert igemm_dispatch(c.shape, "dgrad")["nclass"] == 1
        poison = torch.full_like(x, 1.0)
        del poison
        dx = _C().conv_dgrad_igemm(dy, wT, c.H, c.W, c.stride, c.pad)
        _assert_exact("dx", dx, c.dx.to(dt),
                      _where(igemm_dispatch(c.shape, "dgrad")))
        dx = dx.cpu()
        odd = torch.ones(c.H, c.W, dtype=torch.bool)
        odd[::2, ::2] = False
        assert int(odd.sum()) * 4 == 3 * c.H * c.W
        assert (dx[:, :, odd] == 0).all() and (dx[:, :, ~odd] != 0).any()


# ---- b. forward and input-grad tiles -----------------------------------------

@pytest.mark.parametrize("dt", DTYPES, ids=_ids)
@pytest.mark.parametrize("shape", EXACT_SHAPES, ids=_ids)
def test_fwd_dgrad_tiles_exact(shape, dt):
    """Tiles 64, 128 and 228 each give the reference, so they agree; on the
    split-K shapes tile 228 also runs with 2, 3, 5 and 1000 slices and with
    one more than the pass has reduction tiles (the host clamps)."""
    c = _case(shape)
    ops = c.operands(dt)
    for tile in TILES:
        _fwd_dgrad_exact(c, dt, ops, tile)
    if shape in SPLITK_SHAPES:
        req = {k: splitk_requests(shape, k) for k in ("fwd", "dgrad")}
        for sf, sd in zip(req["fwd"], req["dgrad"]):
            x, w, dy, wT = ops
            y = _C().conv_fwd_igemm(x, w, c.stride, c.pad, 228, sf)
            _assert_exact(f"y tile 228 splits {sf}", y, c.y.to(dt), _where(
                igemm_dispatch(shape, "fwd", 228, sf)))
            dx = _C().conv_dgrad_igemm(dy, wT, c.H, c.W, c.stride, c.pad,
                                       228, sd)
            _assert_exact(f"dx tile 228 splits {sd}", dx, c.dx.to(dt), _where(
                igemm_dispatch(shape, "dgrad", 228, sd)))


# ---- c. weight-grad variants -------------------------------------------------

def _wgrad_pairs_exact(c, dt, pairs):
    x, _, dy, _ = c.operands(dt)
    want = c.dw.to(dt)
    want32 = want.float()
    for wtile, splits in pairs:
        d = wgrad_dispatch(c.shape, wtile, splits)
        tag = (f"wtile {wtile} splits {splits} -> tile {d['tile']} "
               f"{d['TM']}x{d['TN']} grid {d['grid']} {d['path']} "
               f"{d['reduce']}")
        dw = _C().conv_wgrad_igemm(dy, x, c.R, c.R, c.stride, c.pad, splits,
                                   wtile, False)
        _assert_exact(f"dw {tag}", dw, want)
        dw32 = _C().conv_wgrad_igemm(dy, x, c.R, c.R, c.stride, c.pad, splits,
                                     wtile, True)
        _assert_exact(f"dw fp32 {tag}", dw32, want32)


@pytest.mark.parametrize("dt", DTYPES, ids=_ids)
@pytest.mark.parametrize("shape", WGRAD_SHAPES, ids=_ids)
def test_wgrad_variants_exact(shape, dt):
    """Every (wtile, splits) pair gives the reference, the atomic wtile 4
    included, in the 16-bit dtype and widened to fp32: direct stores, slabs
    with each reduce, LIN off 1x1 shapes (falls back to v2), any wtile on the
    generic and the stem shape (falls back to v1), and the wide-stage tiles
    with more slices asked for than they have stages."""
    _wgrad_pairs_exact(_case(shape), dt,
                       [(t, s) for t in WTILES for s in WSPLITS])


@pytest.mark.parametrize("dt", DTYPES, ids=_ids)
def test_wgrad_128_chunks_exact(dt):
    _wgrad_pairs_exact(_case(WGRAD_BIG_SHAPE), dt, WGRAD_BIG_PAIRS)


# ---- d. evaluation epilogue --------------------------------------------------

@pytest.mark.parametrize("dt", DTYPES, ids=_ids)
@pytest.mark.parametrize("shape", BN_SHAPES, ids=_ids)
def test_bn_epilogue_exact(shape, dt):
    """scale in {1, -1, 2, 0.5, 0}, integer shift and residual: conv * scale +
    shift + res is an exact fp32 number (a half-integer at most), so the
    kernel's one rounding must give round(relu(.)) of the CPU's fp32 value."""
    c = _case(shape)
    x, w, _, _ = c.operands(dt)
    K = shape[4]
    g = torch.Generator().manual_seed(59 + K)
    scale = torch.tensor(BN_SCALES)[torch.randint(0, 5, (K,), generator=g)]
    shift = torch.randint(-4, 5, (K,), generator=g).float()
    res = torch.randint(-3, 4, c.y.shape, generator=g).float()
    table = torch.zeros(4, K)
    table[2], table[3] = scale, shift
    table, res_d = table.to(DEV), _dev(res.to(dt))
    pre = c.y * scale.view(1, K, 1, 1) + shift.view(1, K, 1, 1)
    for tile, splits in BN_LAUNCHES:
        where = _where(igemm_dispatch(shape, "fwd_bn", tile, splits))
        for residual, relu in ((None, False), (None, True), (res_d, False),
                               (res_d, True)):
            v = pre if residual is None else pre + res
            want = (v.clamp_min(0) if relu else v).to(dt)
            got = _C().conv_fwd_bn_igemm(x, w, table, residual, relu,
                                         c.stride, c.pad, tile, splits)
            _assert_exact(f"tile {tile} splits {splits} relu {relu} residual "
                          f"{residual is not None}", got, want, where)


# ---- e. public path ----------------------------------------------------------

@pytest.fixture
def no_autotune(monkeypatch):
    monkeypatch.setenv("MI355X_AUTOTUNE", "0")
    return monkeypatch


class _Spy:
    """The extension module, recording each call's name and its arguments
    that are not tensors."""

    def __init__(self, mod):
        self.mod, self.calls = mod, []

    def __getattr__(self, name):
        fn = getattr(self.mod, name)

        def call(*args):
            self.calls.append((name, tuple(
                a for a in args if not isinstance(a, torch.Tensor))))
            return fn(*args)
        return call


def _conv2d_exact(mp, c, dt, igemm=(0,), wgrad=(0, 0)):
    """conv2d() forward and backward give the reference, through the native
    launches with the given (tile[, splits]) and (wtile, splits)."""
    from mi355x_ddp.ops import _backend, conv2d
    spy = _Spy(_C())
    mp.setattr(_backend, "C", lambda: spy)
    x, w, dy, _ = c.operands(dt)
    x.requires_grad_(True)
    w.requires_grad_(True)
    y = conv2d(x, w, (c.stride,) * 2, (c.pad,) * 2)
    y.backward(dy)
    s, p = c.stride, c.pad
    assert spy.calls == [
        ("conv_fwd_igemm", (s, p) + igemm),
        ("conv_build_wT", ()),
        ("conv_dgrad_igemm", (c.H, c.W, s, p) + (igemm + (1,))[:2]),
        ("conv_wgrad_igemm", (c.R, c.R, s, p, wgrad[1], wgrad[0], False)),
    ], spy.calls
    tile = igemm + (1,)
    _assert_exact("y", y.detach(), c.y.to(dt),
                  _where(igemm_dispatch(c.shape, "fwd", *tile[:2])))
    _assert_exact("x.grad", x.grad, c.dx.to(dt),
                  _where(igemm_dispatch(c.shape, "dgrad", *tile[:2])))
    _assert_exact("w.grad", w.grad, c.dw.to(dt))


@pytest.mark.parametrize("dt", DTYPES, ids=_ids)
@pytest.mark.parametrize("shape", PUBLIC_SHAPES, ids=_ids)
def test_public_conv2d_exact(no_autotune, shape, dt):
    no_autotune.setattr(convmod, "_TUNE_CACHE", {})
    _conv2d_exact(no_autotune, _case(shape), dt)
    assert convmod._TUNE_CACHE == {}


# ---- f. tuner pins -----------------------------------------------------------

@pytest.mark.parametrize("dt", DTYPES, ids=_ids)
def test_pinned_choices_exact(no_autotune, dt):
    """The split-K 128x128 tile pinned for the forward and the input-grad and
    the atomic weight-grad pinned in the tuner's cache: conv2d() launches
    them and still gives the reference."""
    N, C, H, W, K, R, stride, pad = PIN_SHAPE
    P, Q = out_extent(PIN_SHAPE)
    xs, ws = torch.Size((N, C, H, W)), torch.Size((K, C, R, R))
    ys, wTs = torch.Size((N, K, P, Q)), torch.Size((C, R, R, K))
    cache = {
        ("fwd", dt, xs, ws, stride, pad): PIN_IGEMM,
        ("dgrad", dt, ys, wTs, stride, pad): PIN_IGEMM,
        ("wgrad_tile", dt, ys, xs, R, stride, pad): PIN_WGRAD,
        ("wgrad_splits", dt, ys, xs, R, stride, pad, PIN_WGRAD[0]): PIN_WGRAD,
    }
    for kind in ("fwd", "dgrad"):
        assert igemm_dispatch(PIN_SHAPE, kind, *PIN_IGEMM)["splits"] == 4
    assert wgrad_dispatch(PIN_SHAPE, *PIN_WGRAD)["path"] == "atomic"
    no_autotune.setattr(convmod, "_TUNE_CACHE", dict(cache))
    _conv2d_exact(no_autotune, _case(PIN_SHAPE), dt, PIN_IGEMM, PIN_WGRAD)
    assert convmod._TUNE_CACHE == cache
