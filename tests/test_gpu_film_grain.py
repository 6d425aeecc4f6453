"""GPU: vvr_read_output_grain on the device (k_film_grain) against the reference's own vvdec::FilmGrain (tests/film_grain_ref.py): the case matrix of
the CPU test on a picture written to a slot, a picture smaller than its slot, 3840x2160 and 7680x4320 10-bit frames, a reconstructed picture read
through Reconstructor.read_output(grain=True) while later pictures are in flight, and the kernel against the host restatement of the stand-in
runtime on banks the reference cannot pin (scale factors up to 255)."""
import ctypes as C

import numpy as np
import pytest

import film_grain_ref
import output_support as SUP
import test_film_grain_host as H
from vvdec_amd import abi, synth, stream

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not film_grain_ref.available(), reason="oracle/_ref/libvvref.so not built (needs /root/reference at build time)")]


def _read(rec, slot, win, bps):
    rc, got = H.read_grain(rec.L, rec.ctx, slot, win, bps, 3 if rec.chroma_format else 1, call=rec.L.vvr_read_output_grain)
    rec._check(rc)
    return got


@pytest.mark.parametrize("cf", [1, 0])
@pytest.mark.parametrize("bd", [10, 8])
def test_matrix_on_the_device(built, tmp_path, bd, cf):
    import vvdec_amd
    picture, steps = film_grain_ref.matrix_sequence(bd, cf)
    banks, want = film_grain_ref.expected(picture, steps, bd, cf, str(tmp_path))
    rec = vvdec_amd.Reconstructor(448, 160, bit_depth=bd, chroma_format=cf, num_slots=3, num_streams=1)
    rec.write_picture(1, picture)
    H.play(rec.set_film_grain, rec.set_film_grain_seed, lambda win, bps: _read(rec, 1, win, bps), steps, banks, want, bd, "k_film_grain")
    # a picture smaller than its slot (vvr_slot_picture_size): windows of that picture; beyond it, inside the slot, refused
    rng = np.random.default_rng(bd + cf)
    small = film_grain_ref.grain_picture(rng, 200, 104, bd, cf)
    banks, want = film_grain_ref.expected(small, [("fgc", film_grain_ref.random_sei(rng, 1, 3, 4, bool(cf))), ("frame", (0, 0, 200, 104), 2),
                                                  ("frame", (4, 2, 160, 96), 2)], bd, cf, str(tmp_path), "small")
    rec._check(rec.L.vvr_slot_picture_size(rec.ctx, 2, 200, 104))
    for c, p in enumerate(small):
        rec._check(rec.L.vvr_write_plane(rec.ctx, 2, c, np.ascontiguousarray(p).ctypes.data, p.shape[1]))
    rec.set_film_grain(banks[0])
    rec.set_film_grain_seed(0xdeadbeef)          # (the reference starts a new chain)
    with pytest.raises(vvdec_amd.VvrError):
        _read(rec, 2, (8, 0, 200, 104), 2)
    for win, w_ in zip([(0, 0, 200, 104), (4, 2, 160, 96)], want):
        got = _read(rec, 2, win, 2)
        assert all(np.array_equal(g, x) for g, x in zip(got, w_)), win
    rec.close()


@pytest.mark.parametrize("size", [(3840, 2160), (7680, 4320)])
def test_headline_sizes(built, tmp_path, size):
    """two 10-bit 4:2:0 frames in a row (the chain carries over) through Reconstructor.read_output(grain=True)"""
    import vvdec_amd
    W, H_ = size
    rng = np.random.default_rng(W)
    planes = synth.natural_picture(W, H_, 7)
    sei = film_grain_ref.random_sei(rng, 0, 8, 5)
    steps = [("fgc", sei), ("frame", (0, 0, W, H_), 2), ("frame", (2, 4, W - 16, H_ - 8), 2)]
    banks, want = film_grain_ref.expected(planes, steps, 10, 1, str(tmp_path), "big")
    rec = vvdec_amd.Reconstructor(W, H_, num_slots=2, num_streams=1)
    rec.write_picture(0, planes)
    rec.set_film_grain(banks[0])
    for (_, win, _), w_ in zip(steps[1:], want):
        got = rec.read_output(0, window=win, grain=True)
        for c in range(3):
            assert np.array_equal(got[c], w_[c]), "%r component %d: %d samples differ" % (win, c, int((got[c] != w_[c]).sum()))
    with pytest.raises(ValueError):
        rec.read_output(0, grain=True, size=(W // 2, H_ // 2))
    rec.close()


@pytest.mark.parametrize("bd", [10, 8])
def test_reconstructed_picture_with_later_pictures_in_flight(built, tmp_path, bd):
    """the grain read of the first picture of a GOP issued while the others are still being reconstructed; then the same window of every picture
    in output order, 8-bit content also as 1-byte samples"""
    import vvdec_amd
    W, H_ = 264, 136
    geo = dict(bit_depth=bd, chroma_format=1, log2_ctu=6)
    plans, nslots = stream.ra_plan(5, gop=4, seed_poc0_is_external=False)
    rec = vvdec_amd.Reconstructor(W, H_, num_slots=nslots, num_streams=2, host_threads=2, **geo)
    tools = abi.TOOL_SAO_LUMA | abi.TOOL_SAO_CHROMA | abi.TOOL_ALF | abi.TOOL_DEP_QUANT | abi.TOOL_MTS | abi.TOOL_LFNST
    rng = np.random.default_rng(bd)
    sei = film_grain_ref.random_sei(rng, 1, 3, 6)
    win = (8, 4, 240, 120)
    jobs = [rec.decompress_picture(synth.picture_for_plan(pl, W, H_, seed=991, tool_flags=tools, **geo)) for pl in plans]
    # the bank comes from the reference, which needs the pictures for nothing: take it first
    banks, _ = film_grain_ref.expected([], [("fgc", sei)], bd, 1, str(tmp_path), "bank")
    rec.set_film_grain(banks[0])
    first = rec.read_output(plans[0].slot, window=win, grain=True)       # (waits for all work on the slot)
    for j in jobs:
        rec.wait(j)
    order = sorted(range(len(plans)), key=lambda k: plans[k].poc)
    pics = [rec.read_picture(plans[k].slot) for k in order]
    x, y, w, h = win
    crop = [[p[c][y >> s:(y + h) >> s, x >> s:(x + w) >> s] for c, s in ((0, 0), (1, 1), (2, 1))] for p in pics]
    # the reference grains the first picture, then every picture in output order, on one FilmGrain
    ops = [["fgc", sei], ["frame", 0, bd, 1]] + [["frame", 1 + n, bd, 1] for n in range(len(order))]
    res = film_grain_ref.run(ops, [crop[order.index(0)]] + crop, str(tmp_path), "recon")
    assert all(np.array_equal(a, b) for a, b in zip(first, res[1])), "the read issued with pictures in flight"
    for n, k in enumerate(order):
        got = rec.read_output(plans[k].slot, window=win, grain=True, bytes_per_sample=1 if bd == 8 and n % 2 else 2)
        for c in range(3):
            w_ = res[2 + n][c].astype(got[c].dtype)
            assert np.array_equal(got[c], w_), "POC %d component %d" % (plans[k].poc, c)
    rec.close()


def _stand_in(bd, cf, picture, cases):
    """(in a child process: the stand-in runtime's library defines the HIP calls it uses) the cases through the stand-in's launch_film_grain"""
    L = SUP.stub_lib()
    ctx = SUP.make_ctx(L, 448, 160, bd, cf)
    SUP.write_picture(L, ctx, 0, picture)
    out, keep = [], []
    for win, bps, bank in cases:
        if bank is not None:
            keep.append(abi.film_grain_bank(**bank))
            assert L.vvr_set_film_grain(ctx, C.addressof(keep[-1])) == abi.VVR_OK
        rc, got = H.read_grain(L, ctx, 0, win, bps, 3 if cf else 1)
        assert rc == abi.VVR_OK, L.vvr_last_error(ctx)
        out.append(got)
    L.vvr_destroy(ctx)
    return out


@pytest.mark.parametrize("cf", [1, 0])
@pytest.mark.parametrize("bd", [10, 8])
def test_kernel_is_the_host_restatement(built, bd, cf):
    """k_film_grain == launch_film_grain of the stand-in runtime on the same inputs, with random banks (every scale factor, eight patterns per
    component, the full int8 range of a pattern) and windows of every width class"""
    import multiprocessing
    import vvdec_amd
    rng = np.random.default_rng(40 + bd + cf)
    picture = film_grain_ref.grain_picture(rng, 448, 160, bd, cf)
    cases = []
    for n, win in enumerate([(0, 0, 448, 160), (2, 2, 130, 34 if cf else 33), (4, 6, 146, 80), (10, 0, 162 if cf else 145, 160), (16, 8, 400, 18 if cf else 17)]):
        bank = None
        if n % 2 == 0:
            bank = H._bank(rng)
            bank["shift"] = int(rng.integers(2, 8))
            bank["comp_present"] = np.array([1, n % 4 == 0, 1], np.uint8)
        cases.append((win, 1 if bd == 8 and n % 2 else 2, bank))
    with multiprocessing.get_context("spawn").Pool(1) as pool:
        want = pool.apply(_stand_in, (bd, cf, picture, cases))
    rec = vvdec_amd.Reconstructor(448, 160, bit_depth=bd, chroma_format=cf, num_slots=1, num_streams=1)
    rec.write_picture(0, picture)
    for (win, bps, bank), w_ in zip(cases, want):
        if bank is not None:
            rec.set_film_grain(bank)
        got = _read(rec, 0, win, bps)
        for c in range(3 if cf else 1):
            assert np.array_equal(got[c], w_[c]), "%r component %d: %d samples differ" % (win, c, int((got[c] != w_[c]).sum()))
    rec.close()
