"""CPU: vvr_read_output_grain, the host half (argument checks, the seed chain, the blocks' random words, the layout of the packed planes, the caller's
strides) on the stand-in runtime of tests/hoststub, whose launch_film_grain is a plain loop restating FilmGrainImpl::add_grain_block
(vvr_output.inc, compiled for the host only).  Ground truth is the reference's own vvdec::FilmGrain (tests/film_grain_ref.py): its banks after
updateFGC, and the frames it grains with prepareBlockSeeds + add_grain_line."""
import ctypes as C

import numpy as np
import pytest

import film_grain_ref
import output_support as SUP
import test_host_glue as T
from vvdec_amd import abi

pytestmark = T.pytestmark
need_ref = pytest.mark.skipif(not film_grain_ref.available(), reason="oracle/_ref/libvvref.so not built (needs /root/reference at build time)")


def read_grain(L, ctx, slot, win, bps, ncomp, pad=(3, 5, 7), call=None):
    """one vvr_read_output_grain call into destinations with padded rows; checks that nothing was written past a row -> (rc, planes)"""
    x, y, w, h = win
    fill = 0xaa if bps == 1 else 0xaaaa
    dt = np.uint8 if bps == 1 else np.uint16
    outs = [np.full((h >> (1 if c else 0), (w >> (1 if c else 0)) + pad[c]), fill, dt) for c in range(ncomp)]
    ptrs = (C.c_void_p * 3)(*[outs[c].ctypes.data if c < ncomp else None for c in range(3)])
    strides = (C.c_size_t * 3)(*[outs[c].strides[0] if c < ncomp else 0 for c in range(3)])
    rc = (call or L.vvr_read_output_grain)(ctx, slot, x, y, w, h, bps, ptrs, strides)
    for c in range(ncomp):
        assert (outs[c][:, outs[c].shape[1] - pad[c]:] == fill).all(), "wrote beyond the row"
    return rc, [o[:, :o.shape[1] - pad[c]] for c, o in enumerate(outs)]


def play(set_bank, set_seed, read, steps, banks, want, bd, what):
    """the steps of film_grain_ref.matrix_sequence against the reference's frames"""
    nb = nf = 0
    for st in steps:
        if st[0] == "fgc":
            set_bank(banks[nb]); nb += 1
        elif st[0] == "seed":
            set_seed(st[1])
        else:
            _, win, bps = st
            got = read(win, bps)
            for c, (g, w_) in enumerate(zip(got, want[nf])):
                w_ = w_.astype(np.uint8) if bps == 1 else w_
                assert g.shape == w_.shape and np.array_equal(g, w_), "%s: frame %d %r (%d bytes) component %d: %d samples differ" % (
                    what, nf, win, bps, c, int((g != w_).sum()))
            nf += 1
    assert nf == len(want)


@need_ref
@pytest.mark.parametrize("cf", [1, 0])
@pytest.mark.parametrize("bd", [10, 8])
def test_sequence_is_the_reference_film_grain(tmp_path, bd, cf):
    """the whole case matrix (film_grain_ref.matrix_sequence) in one sequence on one context, against FilmGrain frame by frame"""
    L = SUP.stub_lib()
    picture, steps = film_grain_ref.matrix_sequence(bd, cf)
    banks, want = film_grain_ref.expected(picture, steps, bd, cf, str(tmp_path))
    ctx = SUP.make_ctx(L, 448, 160, bd, cf)
    SUP.write_picture(L, ctx, 1, picture)
    keep = []

    def set_bank(b):
        keep.append(abi.film_grain_bank(**b))
        assert L.vvr_set_film_grain(ctx, C.addressof(keep[-1])) == abi.VVR_OK

    def read(win, bps):
        rc, got = read_grain(L, ctx, 1, win, bps, 3 if cf else 1)
        assert rc == abi.VVR_OK, L.vvr_last_error(ctx)
        return got
    play(set_bank, lambda s: L.vvr_set_film_grain_seed(ctx, s), read, steps, banks, want, bd, "stand-in")
    L.vvr_destroy(ctx)


@need_ref
def test_a_picture_smaller_than_its_slot(tmp_path):
    """the window is in samples of the picture in the slot (an RPR picture is smaller than the slot): a window beyond that picture is refused"""
    L = SUP.stub_lib()
    rng = np.random.default_rng(5)
    picture = film_grain_ref.grain_picture(rng, 200, 104, 10, 1)
    sei = film_grain_ref.random_sei(rng, 0, 3, 5)
    banks, want = film_grain_ref.expected(picture, [("fgc", sei), ("frame", (0, 0, 200, 104), 2), ("frame", (4, 2, 160, 96), 2)], 10, 1, str(tmp_path))
    ctx = SUP.make_ctx(L, 448, 160, 10, 1)
    assert L.vvr_slot_picture_size(ctx, 0, 200, 104) == abi.VVR_OK
    for c, p in enumerate(picture):
        assert L.vvr_write_plane(ctx, 0, c, np.ascontiguousarray(p).ctypes.data, p.shape[1]) == abi.VVR_OK
    bank = abi.film_grain_bank(**banks[0])
    assert L.vvr_set_film_grain(ctx, C.addressof(bank)) == abi.VVR_OK
    assert read_grain(L, ctx, 0, (8, 0, 200, 104), 2, 3)[0] == abi.VVR_ERR_PARAMETER      # (inside the slot)
    for win, w_ in zip([(0, 0, 200, 104), (4, 2, 160, 96)], want):
        rc, got = read_grain(L, ctx, 0, win, 2, 3)
        assert rc == abi.VVR_OK and all(np.array_equal(g, x) for g, x in zip(got, w_))
    L.vvr_destroy(ctx)


def _bank(rng):
    b = dict(comp_present=np.ones(3, np.uint8), shift=4, scale_lut=rng.integers(0, 256, (3, 256)).astype(np.uint8),
             pattern_lut=(rng.integers(0, 8, (3, 256)) << 4).astype(np.uint8), pattern=rng.integers(-127, 128, (2, 8, 64, 64)).astype(np.int8))
    return b


def test_refusals_and_the_chain():
    """every refusal of vvr_set_film_grain / vvr_read_output_grain, with a message; a refused read does not advance the seed chain; the chain
    starts at 0xdeadbeef, vvr_set_film_grain does not touch it and vvr_set_film_grain_seed sets it"""
    L = SUP.stub_lib()
    rng = np.random.default_rng(9)
    ctx = SUP.make_ctx(L, 448, 160, 10, 1)
    SUP.write_picture(L, ctx, 0, film_grain_ref.grain_picture(rng, 448, 160, 10, 1))
    win = (2, 4, 200, 64)
    assert read_grain(L, ctx, 0, win, 2, 3)[0] == abi.VVR_ERR_PARAMETER and b"no film grain bank" in L.vvr_last_error(ctx)
    good = _bank(rng)
    bank = abi.film_grain_bank(**good)
    for field, value in (("struct_size", C.sizeof(bank) - 1), ("shift", 1), ("shift", 8)):
        bad = abi.film_grain_bank(**good)
        setattr(bad, field, value)
        assert L.vvr_set_film_grain(ctx, C.addressof(bad)) == abi.VVR_ERR_PARAMETER and L.vvr_last_error(ctx), (field, value)
    lut = good["pattern_lut"].copy()
    lut[2, 77] = 0x80
    bad = abi.film_grain_bank(**dict(good, pattern_lut=lut))
    assert L.vvr_set_film_grain(ctx, C.addressof(bad)) == abi.VVR_ERR_PARAMETER and b"pattern_lut" in L.vvr_last_error(ctx)
    assert read_grain(L, ctx, 0, win, 2, 3)[0] == abi.VVR_ERR_PARAMETER      # (the refused banks left none)
    assert L.vvr_set_film_grain(ctx, C.addressof(bank)) == abi.VVR_OK
    for bad_win, bps in [((0, 0, 128, 64), 2), ((0, 0, 100, 64), 2),                                   # width <= 128
                         ((1, 0, 200, 64), 2), ((0, 1, 200, 64), 2), ((0, 0, 201, 64), 2), ((0, 0, 200, 63), 2),   # odd in 4:2:0
                         ((300, 0, 200, 64), 2), ((0, 120, 200, 64), 2), ((-2, 0, 200, 64), 2), ((0, 0, 200, 0), 2),   # outside
                         (win, 1), (win, 3)]:                                                             # 1 byte of 10 bits, sample size
        assert read_grain(L, ctx, 0, bad_win, bps, 3)[0] == abi.VVR_ERR_PARAMETER and L.vvr_last_error(ctx), (bad_win, bps)
    # a stride below the row, a missing plane
    buf = np.zeros(200 * 64, np.uint16)
    ptrs = (C.c_void_p * 3)(buf.ctypes.data, buf.ctypes.data, buf.ctypes.data)
    assert L.vvr_read_output_grain(ctx, 0, *win, 2, ptrs, (C.c_size_t * 3)(400, 199, 200)) == abi.VVR_ERR_PARAMETER
    assert L.vvr_read_output_grain(ctx, 0, *win, 2, (C.c_void_p * 3)(buf.ctypes.data, None, buf.ctypes.data), (C.c_size_t * 3)(400, 200, 200)) == abi.VVR_ERR_PARAMETER
    # none of that advanced the chain: the next frame is the first frame of a fresh context
    rc, first = read_grain(L, ctx, 0, win, 2, 3)
    assert rc == abi.VVR_OK
    ctx2 = SUP.make_ctx(L, 448, 160, 10, 1)
    SUP.write_picture(L, ctx2, 0, film_grain_ref.grain_picture(np.random.default_rng(9), 448, 160, 10, 1))
    assert L.vvr_set_film_grain(ctx2, C.addressof(bank)) == abi.VVR_OK
    rc, again = read_grain(L, ctx2, 0, win, 2, 3)
    assert rc == abi.VVR_OK and all(np.array_equal(a, b) for a, b in zip(first, again))
    # the chain moved on (a second frame differs), setting the bank again does not reset it, setting the seed to 0xdeadbeef does
    assert L.vvr_set_film_grain(ctx2, C.addressof(bank)) == abi.VVR_OK
    rc, second = read_grain(L, ctx2, 0, win, 2, 3)
    assert rc == abi.VVR_OK and not np.array_equal(second[0], first[0])
    assert L.vvr_set_film_grain_seed(ctx2, 0xdeadbeef) == abi.VVR_OK
    rc, third = read_grain(L, ctx2, 0, win, 2, 3)
    assert rc == abi.VVR_OK and all(np.array_equal(a, b) for a, b in zip(first, third))
    assert L.vvr_set_film_grain(ctx2, None) == abi.VVR_OK
    assert read_grain(L, ctx2, 0, win, 2, 3)[0] == abi.VVR_ERR_PARAMETER
    L.vvr_destroy(ctx2)
    # bit depths other than 8 and 10
    ctx9 = SUP.make_ctx(L, 448, 160, 9, 1)
    assert L.vvr_set_film_grain(ctx9, C.addressof(bank)) == abi.VVR_OK
    assert read_grain(L, ctx9, 0, win, 2, 3)[0] == abi.VVR_ERR_PARAMETER and b"bit depth" in L.vvr_last_error(ctx9)
    L.vvr_destroy(ctx9)
    L.vvr_destroy(ctx)
