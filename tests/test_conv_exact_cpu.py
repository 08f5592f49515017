"""What tests/test_conv_exact_gpu.py launches, checked without a GPU: its
plain-Python mirror of the host dispatch of csrc/conv_igemm.hip against
hand-worked launches, its shape lists against the full set of kernel
instantiations the host can launch (each reached on more than one tile with a
ragged edge), the named targets of its shape table, and the operand bounds and
the wide-range share of every reference."""
import importlib.util
import os

import pytest
import torch


def _exact_module():
    """The GPU test module, loaded by path: it holds the shape lists and the
    mirror of the host dispatch."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                        "test_conv_exact_gpu.py")
    spec = importlib.util.spec_from_file_location("_conv_exact", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def mod():
    return _exact_module()


# conv_igemm_kernel<T, MODE, FAST, BMT, PADC, BNT, SPLITK, BNEPI>, as the host
# of conv_fwd_igemm, conv_fwd_bn_igemm and conv_dgrad_igemm instantiates it
def _all_igemm():
    out = []
    for bnepi in (False, True):
        for bmt in (64, 128):
            out += [(0, False, bmt, True, 64, False, bnepi),     # PADC stem
                    (0, True, bmt, False, 64, False, bnepi),     # FAST
                    (0, False, bmt, False, 64, False, bnepi)]    # generic
        out.append((0, True, 128, False, 128, False, bnepi))     # tile 228
    out.append((0, True, 128, False, 128, True, False))          # split-K
    for bmt in (64, 128):
        out += [(1, True, bmt, False, 64, False, False),
                (1, False, bmt, False, 64, False, False),
                (2, True, bmt, False, 64, False, False)]
    out += [(1, True, 128, False, 128, False, False),
            (1, True, 128, False, 128, True, False)]
    return out


ALL_IGEMM = _all_igemm()
IGEMM_REDUCES = [("igemm", False), ("igemm", True)]

# conv_wgrad_kernel<T, FAST, PADC, DIRECT, ATOMIC>,
# conv_wgrad_v2_kernel<T, WGM, WGN, DIRECT, CH>,
# conv_wgrad_lin_kernel<T, WGM, WGN, DIRECT>
ALL_WGRAD = (
    [("v1", True, False, True, False), ("v1", False, False, True, False),
     ("v1", False, True, False, True), ("v1", True, False, False, True),
     ("v1", False, False, False, True), ("v1", False, True, False, False),
     ("v1", True, False, False, False), ("v1", False, False, False, False)] +
    [("v2", wgm, wgn, direct, ch) for wgm, wgn in ((2, 2), (4, 1))
     for direct in (True, False) for ch in (1, 2)] +
    [("lin", wgm, wgn, direct) for wgm, wgn in ((2, 2), (4, 1))
     for direct in (True, False)])
# wgrad_reduce_kernel and wgrad_reduce_frag_kernel<T, ZW, V>
WGRAD_REDUCES = [("rowmajor",), ("frag", 1, 1), ("frag", 1, 4),
                 ("frag", 2, 4), ("frag", 4, 4), ("frag", 8, 4),
                 ("frag", 16, 4)]


def test_the_instantiation_lists_are_complete():
    assert len(ALL_IGEMM) == len(set(ALL_IGEMM)) == 23
    assert len(ALL_WGRAD) == len(set(ALL_WGRAD)) == 20


# ---- the mirror against launches worked out by hand from the host code -------

def test_igemm_mirror_on_known_shapes(mod):
    d = mod.igemm_dispatch
    # stage-1 3x3 of the CIFAR ResNet at batch 8: 64 x 1 tiles of 128 < 384
    r = d((8, 64, 32, 32, 64, 3, 1, 1), "fwd")
    assert r["inst"] == (0, True, 64, False, 64, False, False)
    assert (r["M"], r["N"], r["K"], r["grid"]) == (8192, 64, 576, (1, 128, 1))
    # batch 256: 2048 tiles of 128 -> the 128 tile
    assert d((256, 64, 32, 32, 64, 3, 1, 1), "fwd")["inst"][2] == 128
    # stem: reduction 27 -> 9 taps x 4 channels = 36 -> 64; 7x7: 196 -> 256
    r = d((8, 3, 32, 32, 64, 3, 1, 1), "fwd", 128)
    assert r["inst"] == (0, False, 128, True, 64, False, False)
    assert (r["K"], r["grid"]) == (64, (1, 64, 1))
    assert d((4, 3, 64, 64, 64, 7, 2, 3), "fwd")["K"] == 256
    # stage-4 3x3 at batch 8: M = 128, 72 reduction tiles
    s4 = (8, 512, 4, 4, 512, 3, 1, 1)
    r = d(s4, "fwd", 228, 4)
    assert r["inst"] == (0, True, 128, False, 128, True, False)
    assert (r["grid"], r["splits"], r["reduce"]) == \
        ((4, 1, 4), 4, ("igemm", False))
    assert d(s4, "fwd", 228, 1000)["splits"] == 72
    assert d(s4, "fwd", 228, 1)["inst"] == \
        (0, True, 128, False, 128, False, False)
    assert d(s4, "fwd", 128, 4)["splits"] == 1        # splits need tile 228
    assert d(s4, "fwd_bn", 228, 4)["reduce"] == ("igemm", True)
    assert d(s4, "fwd_bn", 228, 1)["inst"][6] is True
    assert d(s4, "dgrad", 228, 2)["inst"] == \
        (1, True, 128, False, 128, True, False)
    # stride-2 3x3 with even extents: four parity classes of M / 4 rows
    r = d((8, 64, 32, 32, 128, 3, 2, 1), "dgrad", 228, 4)
    assert r["inst"] == (2, True, 64, False, 64, False, False)
    assert (r["M"], r["N"], r["K"], r["nclass"], r["grid"], r["splits"]) == \
        (2048, 64, 1152, 4, (1, 32, 4), 1)
    # 1x1 stride 2: one class over a memset
    r = d((8, 64, 32, 32, 128, 1, 2, 0), "dgrad", 128)
    assert (r["nclass"], r["grid"]) == (1, (1, 16, 1))
    # odd extents: the plain MODE 1 kernel
    r = d((3, 64, 9, 13, 128, 3, 2, 1), "dgrad")
    assert r["inst"][0] == 1 and r["nclass"] == 0 and r["M"] == 3 * 9 * 13
    # K = 100: the input-grad gathers 100 channels, not a multiple of 64
    assert d((2, 64, 8, 12, 100, 3, 1, 1), "dgrad", 228, 4)["inst"] == \
        (1, False, 64, False, 64, False, False)
    # N = 64 < 96 never takes the 128-wide N tile
    assert d((8, 64, 32, 32, 64, 3, 1, 1), "fwd", 228, 4)["inst"][4] == 64


def test_wgrad_mirror_on_known_shapes(mod):
    d = mod.wgrad_dispatch
    s1 = (8, 64, 32, 32, 64, 3, 1, 1)     # M = 64, N = 576, 128 chunks
    r = d(s1)
    assert (r["tile"], r["TM"], r["TN"], r["grid"]) == (1, 64, 128, (5, 1, 16))
    assert r["kernel"] == ("v1", True, False, False, False)
    assert (r["path"], r["reduce"]) == ("slab", ("frag", 1, 1))
    assert d(s1, 1, 1)["kernel"] == ("v1", True, False, True, False)
    assert d(s1, 1, 1)["reduce"] is None
    assert d(s1, 1, 128)["reduce"] == ("frag", 16, 4)
    assert d(s1, 1, 1000)["splits"] == 128
    assert d(s1, 1, -1)["splits"] == 16               # min(1024 / 5, 128 / 8)
    assert d(s1, 8, 1000)["splits"] == 64             # 64 stages of 128 rows
    assert d(s1, 8, 1000)["kernel"] == ("v2", 2, 2, False, 2)
    assert d(s1, 5, 0)["tile"] == 2                   # LIN needs a 1x1 filter
    assert d(s1, 4, 1)["path"] == "atomic"            # even with one slice
    assert d(s1, 4, 1)["reduce"] == ("rowmajor",)
    # resnet50 1x1 expand, M = 256, N = 64: LIN 256x64 by the heuristic
    e = (8, 64, 32, 32, 256, 1, 1, 0)
    r = d(e)
    assert (r["tile"], r["TM"], r["TN"]) == (6, 256, 64)
    assert r["kernel"] == ("lin", 4, 1, False)
    assert d((8, 128, 16, 16, 256, 1, 1, 0))["tile"] == 5
    assert d((8, 128, 16, 16, 128, 3, 1, 1))["tile"] == 2
    assert d((8, 64, 32, 32, 256, 3, 1, 1), 0, 0)["tile"] == 2   # N = 576
    # the stem: any wtile is v1 PADC, never direct; 36 padded columns
    st = (8, 3, 32, 32, 64, 3, 1, 1)
    for wtile in (0, 2, 6, 9):
        r = d(st, wtile, 1)
        assert r["kernel"] == ("v1", False, True, False, False)
        assert (r["N"], r["path"], r["splits"]) == (36, "slab", 1)
    assert d(st, 4, 1)["kernel"] == ("v1", False, True, False, True)
    # K % 16 != 0 falls off FAST whatever C is
    assert d((2, 64, 8, 12, 100, 3, 1, 1), 2, 1)["kernel"] == \
        ("v1", False, False, True, False)


# ---- the named targets of the shape table ------------------------------------

def test_shape_table_reaches_its_named_targets(mod):
    d, w = mod.igemm_dispatch, mod.wgrad_dispatch
    S = mod.EXACT_SHAPES
    # no square image but the 1 x 1 one (and section c's one large case)
    assert all(s[2] != s[3] for s in S[:20] + mod.WGRAD_SHAPES +
               mod.WIDE_SHAPES)
    r = d(S[0], "fwd")
    assert r["inst"][1] and r["M"] == 252 and 252 % 64 and 252 % 128
    r = d(S[1], "dgrad")
    assert (r["inst"][0], r["nclass"], r["M"]) == (2, 4, 105)
    assert d(S[1], "fwd", 228)["inst"][4] == 128
    assert d(S[2], "dgrad")["inst"][:2] == (1, True) and S[2][6] == 2
    assert d(S[3], "dgrad")["nclass"] == 1
    for s in (S[4], S[5]):
        assert {d(s, "fwd", t)["inst"][2:4] for t in (64, 128)} == \
            {(64, True), (128, True)}
    assert d(S[5], "fwd")["K"] == 256
    assert d(S[6], "fwd", 228)["inst"][4] == 128
    assert w(S[6])["kernel"] == ("lin", 2, 2, True)
    assert w(S[7])["kernel"] == ("lin", 4, 1, True) and d(S[7], "fwd")["M"] \
        == 640
    r = d(S[8], "fwd", 228, 1000)
    assert (r["M"], r["K"] // 64, r["splits"]) == (48, 36, 36)
    assert d(S[8], "dgrad", 228, 2)["inst"][5]
    assert (w(S[8])["kernel"], w(S[8])["grid"][:2]) == \
        (("v2", 2, 2, True, 1), (18, 4))
    r = d(S[9], "fwd", 228, 2)
    assert r["inst"][5] and r["grid"] == (2, 2, 2) and r["M"] % 128
    r = d(S[10], "fwd", 228, 3)
    assert r["inst"][5] and r["N"] == 100 and r["N"] % 8
    assert not d(S[10], "dgrad")["inst"][1]
    assert w(S[10])["kernel"][1] is False
    for s in (S[11], S[12], S[13], S[14]):
        assert not d(s, "fwd")["inst"][1] and not d(s, "fwd")["inst"][3]
        assert not d(s, "dgrad")["inst"][1]
        assert w(s)["kernel"][:3] == ("v1", False, False)
    for s in (S[11], S[12]):
        r = d(s, "fwd")
        assert r["M"] % 64 and r["N"] % 64 and r["K"] % 64
    assert [s[1] for s in (S[13], S[14])] == [1, 4]
    assert [(s[5], s[6], s[7]) for s in S[15:19]] == \
        [(3, 1, 0), (1, 1, 1), (5, 3, 2), (3, 2, 0)]
    r = d(S[18], "dgrad")                 # parity classes with P < H / 2
    assert r["inst"][0] == 2 and mod.out_extent(S[18])[0] < S[18][2] // 2
    assert (S[19][2], S[20][2:4]) == (1, (1, 1))
    # section b's split shapes split in the passes the table names
    for s in mod.SPLITK_SHAPES:
        assert d(s, "fwd", 228, 2)["inst"][5]
    assert [d(s, "dgrad", 228, 2)["inst"][5] for s in mod.SPLITK_SHAPES] == \
        [True, True, False]
    for s in mod.SPLITK_SHAPES[:2]:
        for kind in ("fwd", "dgrad"):
            tiles = d(s, kind)["K"] // 64
            req = mod.splitk_requests(s, kind)
            assert req[-1] == tiles + 1 and 5 < tiles < 1000
            assert [d(s, kind, 228, n)["splits"] for n in req] == \
                [2, 3, 5, tiles, tiles]
    # section c: a ragged second M tile on the 128-row and the 256-row tile,
    # for v2 on the first shape and for LIN on the second
    for shape, wtiles in ((mod.WGRAD_SHAPES[0], (2, 3, 8, 9)),
                          (mod.WGRAD_SHAPES[1], (5, 6))):
        for wtile in wtiles:
            r = w(shape, wtile, 2)
            assert r["tile"] == wtile and r["grid"][1] > 1
            assert r["M"] % r["TM"] != 0, (shape, wtile)
    r = w(mod.WGRAD_SHAPES[0], 2, 1)
    assert (r["grid"][:2], r["N"] % 128) == ((5, 3), 64)
    assert w(mod.WGRAD_SHAPES[1], 5, 1)["N"] % 128 == 64
    # the large case has the 128 chunks ZW = 16 needs, and every pair uses them
    assert w(mod.WGRAD_BIG_SHAPE)["K"] == 128 * 64
    for wtile, splits in mod.WGRAD_BIG_PAIRS:
        r = w(mod.WGRAD_BIG_SHAPE, wtile, splits)
        assert r["splits"] >= 16 or r["path"] == "atomic", (wtile, splits)
    # section d: FAST, generic, stem, split-K with N = 100
    kinds = [d(s, "fwd_bn", 228, 3)["inst"] for s in mod.BN_SHAPES]
    assert [(i[1], i[3], i[5]) for i in kinds] == [
        (True, False, False), (False, False, False), (False, True, False),
        (True, False, True)]
    # section f pins launches that differ from the defaults
    for kind in ("fwd", "dgrad"):
        assert d(mod.PIN_SHAPE, kind, *mod.PIN_IGEMM)["inst"][5]
    assert w(mod.PIN_SHAPE, *mod.PIN_WGRAD)["path"] == "atomic"


# ---- every instantiation is reached, on more than one tile, with an edge -----

def _multi_and_ragged(grid, M, N, bm, bn):
    return grid[0] * grid[1] > 1 and (M % bm != 0 or N % bn != 0)


def test_every_igemm_instantiation_is_launched(mod):
    reached, good, reduces = {}, {}, set()
    for section, shape, kind, tile, splits in mod.launched_igemm():
        r = mod.igemm_dispatch(shape, kind, tile, splits)
        inst = r["inst"]
        assert inst in ALL_IGEMM, (shape, kind, tile, splits, inst)
        reached.setdefault(inst, set()).add(section)
        if r["reduce"]:
            reduces.add(r["reduce"])
        if _multi_and_ragged(r["grid"], r["M"], r["N"], inst[2], inst[4]):
            good.setdefault(inst, []).append((section, shape, kind, tile))
    for inst in ALL_IGEMM:
        print(inst, "sections", sorted(reached.get(inst, ())),
              "multi-tile and ragged:", len(good.get(inst, ())))
    missing = [i for i in ALL_IGEMM if i not in reached]
    assert not missing, f"no case launches {missing}"
    weak = [i for i in ALL_IGEMM if i not in good]
    assert not weak, f"launched on one tile or without a ragged edge: {weak}"
    assert reduces == set(IGEMM_REDUCES)
    # the split-K reduce runs with N % 8 == 0 (vector stores) and without
    vec = {mod.igemm_dispatch(s, k, t, z)["N"] % 8 == 0
           for _, s, k, t, z in mod.launched_igemm()
           if mod.igemm_dispatch(s, k, t, z)["reduce"]}
    assert vec == {True, False}
    # the parity kernel runs with four classes and with one
    assert {mod.igemm_dispatch(s, k, t, z)["nclass"]
            for _, s, k, t, z in mod.launched_igemm()} == {0, 1, 4}


def test_every_wgrad_kernel_and_reduce_is_launched(mod):
    reached, good, reduces = set(), set(), set()
    for section, shape, wtile, splits in mod.launched_wgrad():
        r = mod.wgrad_dispatch(shape, wtile, splits)
        assert r["kernel"] in ALL_WGRAD, (shape, wtile, splits, r)
        reached.add(r["kernel"])
        multi = _multi_and_ragged(r["grid"], r["M"], r["N"], r["TM"], r["TN"])
        if multi:
            good.add(r["kernel"])
        if r["reduce"]:
            reduces.add(r["reduce"])
            if multi:
                good.add(r["reduce"])
    missing = [k for k in ALL_WGRAD if k not in reached]
    assert not missing, f"no case launches {missing}"
    weak = [k for k in ALL_WGRAD + WGRAD_REDUCES if k not in good]
    assert not weak, f"launched on one tile or without a ragged edge: {weak}"
    assert reduces == set(WGRAD_REDUCES)
    # more than one tile along M for both tile heights of v2 and LIN
    for fam, tm, shape, wtile in (("v2", 128, 0, 2), ("lin", 128, 1, 5),
                                  ("lin", 256, 1, 6), ("v2", 256, 1, 3)):
        r = mod.wgrad_dispatch(mod.WGRAD_SHAPES[shape], wtile, 2)
        if fam == "v2" and tm == 256:      # a LIN shape asked for plain v2
            assert r["kernel"][0] == "v2"
        assert r["kernel"][0] == fam and r["TM"] == tm and r["grid"][1] > 1


# ---- the references: operand bounds and the wide-range share -----------------

def test_references_are_exact_and_in_range(mod):
    """_Case asserts |y|, |dx|, |dw| < 2^24 and < 65504 and that each has
    non-zero elements; here every shape of the GPU file is built once."""
    shapes = {s for _, s, *_ in mod.launched_igemm()} | \
        {s for _, s, *_ in mod.launched_wgrad()}
    assert len(shapes) >= len(mod.EXACT_SHAPES) + 3
    for shape in sorted(shapes):
        wide = shape in mod.WIDE_SHAPES
        c = mod._case(shape, 15, 15) if wide else mod._case(shape)
        amax, wmax = (15, 15) if wide else (3, 2)
        for t, bound in ((c.x, amax), (c.dy, amax), (c.w, wmax)):
            assert t.abs().max() == bound and torch.equal(t, t.round())
        for dt in mod.DTYPES:       # the operands are exact in both formats
            for t in (c.x, c.w, c.dy):
                assert torch.equal(t.to(dt).float(), t)


def test_wide_operands_round_in_both_formats(mod):
    """At least a tenth of every pass's reference lies beyond 2048 in
    magnitude, where neither bf16 nor fp16 holds every integer, and some of it
    changes under the rounding in each format."""
    kinds = set()
    for shape in mod.WIDE_SHAPES:
        c = mod._case(shape, 15, 15)
        kinds.add(mod.igemm_dispatch(shape, "fwd")["inst"][1])
        for name, ref in (("y", c.y), ("dx", c.dx), ("dw", c.dw)):
            share = (ref.abs() > 2048).float().mean().item()
            print(shape, name, f"share beyond 2048: {share:.3f}",
                  f"max {ref.abs().max().item():.0f}")
            assert share >= 0.1, (shape, name, share)
            for dt in mod.DTYPES:
                assert (ref.to(dt).float() != ref).any(), (shape, name, dt)
    assert kinds == {True, False}          # one FAST, one generic
