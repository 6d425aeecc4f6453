"""The host stage of an I picture built by the worker threads together (vvdec_amd/csrc/vvr_prepare.cpp, buildIntraInParts): two parallel phases over
bands of CTU rows - the per-block work of the unit and item tables inside the bands, a join that only adds up the bands' totals - must send the device
byte for byte what one thread sends.  Runs against the stand-in HIP runtime (tests/hoststub), no GPU.

What is compared: the hash of everything copied to the device for the picture (vvt_take_h2d_hash: CU / TU records, transform blocks, intra items, unit
table, chroma scaling VPDUs, ...), host_threads in {2, 3, 8, 32} against host_threads = 0.  The stand-in's vvt_intra_tables reads the tables of a
vvr_prepare handle, which one thread builds whatever the context's host_threads: they are compared too (a context with worker threads prepares handles
like one without), and they are what the preconditions of every case are checked on - a picture that misses them would silently not be built in bands."""
import ctypes as C

import numpy as np
import pytest

from vvdec_amd import abi, synth, stream
from test_host_glue import build_stub, UNIT_DT, ITEM_DT, TOOLS, HIP_INC
import os

pytestmark = pytest.mark.skipif(not os.path.exists(os.path.join(HIP_INC, "hip", "hip_runtime_api.h")), reason="HIP headers not installed")

THREADS = (2, 3, 8, 32)            # 32: more threads than CTU rows at every size below
T_LMCS = TOOLS | abi.TOOL_LMCS | abi.TOOL_LMCS_CSCALE

# (name, W, H, log2 CTU, seed, generator settings, large blocks wanted at band edges)
CASES = [
    # two CTU rows: the smallest picture that is split at all; dual tree with CCLM, small CUs so that there are 512 of them
    ("two_rows_dual_tree_cclm", 384, 256, 7, 9101, dict(dual_tree=1.0, p_cclm=0.4, p_split_scale=2.0), False),
    # three rows; ISP and MIP (CUs down to 4 x 4: 512 CUs in twelve CTUs)
    ("three_rows_isp_mip", 256, 192, 6, 9102, dict(p_isp=0.3, p_mip=0.3, p_cclm=0.2, p_split_scale=3.0, min_cu_log2=2), False),
    # eight rows, the last one partial (240 = 7.5 x 32)
    ("eight_rows_last_partial", 416, 240, 5, 9103, dict(dual_tree=1.0, p_cclm=0.3, p_isp=0.2, p_mip=0.2, p_split_scale=2.0), False),
    # nine rows, the last one partial; large CUs: blocks of 512 .. 4096 samples (2, 4 or 8 items each) first and last in a band
    ("1080p_large_cus", 1920, 1080, 7, 9104, dict(p_cclm=0.3, p_isp=0.1, p_mip=0.1, p_split_scale=0.55), True),
]


@pytest.fixture(scope="module")
def stub():
    L = abi.bind(C.CDLL(build_stub()))
    L.vvt_intra_tables.argtypes = [C.c_void_p] + [C.c_void_p] * 4
    L.vvt_take_h2d_hash.restype = C.c_ulonglong
    L.vvt_sizeof.restype = C.c_size_t
    assert L.vvt_sizeof(0) == UNIT_DT.itemsize and L.vvt_sizeof(1) == ITEM_DT.itemsize
    return L


def _context(L, W, H, l2, threads):
    cfg = abi.Config()
    cfg.abi_version = abi.VVR_ABI_VERSION
    cfg.device, cfg.max_width, cfg.max_height, cfg.chroma_format, cfg.bit_depth, cfg.log2_ctu = 0, W, H, 1, 10, l2
    cfg.num_slots, cfg.num_streams, cfg.host_threads = 4, 2, threads
    ctx = C.c_void_p()
    assert L.vvr_create(C.byref(cfg), C.byref(ctx)) == abi.VVR_OK
    return ctx


def _i_picture(W, H, l2, seed, tools=T_LMCS, **kw):
    plans, _ = stream.ra_plan(1, gop=1, seed_poc0_is_external=False)
    assert plans[0].slice_type == abi.SLICE_I
    return synth.picture_for_plan(plans[0], W, H, seed=seed, tool_flags=tools, log2_ctu=l2, **kw)


def _upload(L, d, threads):
    """the picture through vvr_submit of a context with `threads` workers, and through vvr_prepare of the same context:
    (hash of all bytes copied to the device by the submission, units, items of the handle)"""
    h = d.hdr
    ctx = _context(L, h.width, h.height, h.log2_ctu, threads)
    p = d.c()
    L.vvt_take_h2d_hash()
    j = L.vvr_submit(ctx, C.byref(p))
    assert j >= 0 and L.vvr_wait(ctx, j) == abi.VVR_OK, L.vvr_last_error(ctx).decode()
    hsh = L.vvt_take_h2d_hash()
    q = C.c_void_p()
    assert L.vvr_prepare(ctx, C.byref(p), C.byref(q)) == abi.VVR_OK, L.vvr_last_error(ctx).decode()
    up, ip, nu, ni = C.c_void_p(), C.c_void_p(), C.c_int(), C.c_int()
    assert L.vvt_intra_tables(q, C.byref(up), C.byref(nu), C.byref(ip), C.byref(ni)) == 0
    units = np.frombuffer((C.c_char * (UNIT_DT.itemsize * nu.value)).from_address(up.value), UNIT_DT).copy()
    items = np.frombuffer((C.c_char * (ITEM_DT.itemsize * ni.value)).from_address(ip.value), ITEM_DT).copy()
    L.vvr_free_prepared(ctx, q)
    L.vvr_destroy(ctx)
    return hsh, units, items


def _band_edges(d, units, items, threads):
    """(items the block behind a band boundary has, items the block in front of it has) for every boundary between the bands `threads` workers build,
    luma: from the unit of the band's first CTU and of the last CTU of the band before"""
    h = d.hdr
    ctu = 1 << h.log2_ctu
    ctusX, ctusY = (h.width + ctu - 1) // ctu, (h.height + ctu - 1) // ctu
    n = min(threads, ctusY)
    by_ctu = {(int(u["ent"]) >> 24 & 3, int(u["ent"]) & 0xffffff): u for u in units if u["i1"] > u["i0"]}
    out = []
    for part in range(1, n):
        row0 = ctusY * part // n
        first, last = by_ctu[(0, row0 * ctusX)], by_ctu[(0, row0 * ctusX - 1)]
        out.append((1 << (int(items[int(first["i0"])]["nTL"]) >> 4), 1 << (int(items[int(last["i1"]) - 1]["nTL"]) >> 4)))
    return out


@pytest.mark.parametrize("name,W,H,l2,seed,kw,large", CASES, ids=[c[0] for c in CASES])
def test_bands_upload_what_one_thread_uploads(stub, name, W, H, l2, seed, kw, large):
    d = _i_picture(W, H, l2, seed, **kw)
    # ---- preconditions of the path (vvr_host_build): enough CUs, two CTU rows, every CU an intra CU, no intra block copy
    ctu = 1 << l2
    assert len(d.cu) >= 512, "%s: %d CUs - the picture would not be built in bands" % (name, len(d.cu))
    assert (H + ctu - 1) // ctu >= 2 and d.ctu_first_cu is not None
    assert not (d.hdr.tool_flags & abi.TOOL_IBC) and np.all(d.cu["pred_mode"] == abi.PRED_INTRA)
    one, units1, items1 = _upload(stub, d, 0)
    # ---- what the case is there for
    assert d.hdr.tool_flags & abi.TOOL_LMCS_CSCALE and np.any((items1["comp"] & 3) > 0)             # chroma blocks, scaled: every band has csVpdu entries
    if "dual_tree" in kw:
        assert np.any((d.cu["tree"] == abi.TREE_CHROMA) & (d.cu["intra_dir"][:, 1] >= 67) & (d.cu["intra_dir"][:, 1] <= 69)), "no CCLM CU in a chroma tree"
    if kw.get("p_isp", 0) >= 0.3:
        assert np.any(d.cu["isp_mode"] > 0) and np.any(d.cu["flags"].astype(int) & abi.CU_MIP), "no ISP / MIP CU"
    if large:
        lp = items1["nTL"].astype(int) >> 4
        assert {1, 2, 3} <= set(np.unique(lp).tolist()), "blocks of 2, 4 and 8 items wanted"
        edges = [e for t in THREADS for e in _band_edges(d, units1, items1, t)]
        assert any(a > 1 for a, b in edges) and any(b > 1 for a, b in edges), "no multi-item block first / last in a band: %r" % (edges,)
    for threads in THREADS:
        hsh, units, items = _upload(stub, d, threads)
        assert hsh == one, "%s: %d threads upload other bytes than one thread" % (name, threads)
        assert units.tobytes() == units1.tobytes() and items.tobytes() == items1.tobytes(), (name, threads)


def test_a_bad_record_in_the_last_band_fails_like_with_one_thread(stub):
    """a record broken in the last band (cu.w = 0): same code, same message as from one thread - and an earlier band's error goes first"""
    W, H, l2 = 416, 240, 5
    d = _i_picture(W, H, l2, 9103, dual_tree=1.0, p_cclm=0.3, p_isp=0.2, p_mip=0.2, p_split_scale=2.0)
    assert len(d.cu) >= 512
    last_row_first_cu = int(d.ctu_first_cu[((H + 31) // 32 - 1) * ((W + 31) // 32)])
    k = len(d.cu) - 3
    assert k >= last_row_first_cu                         # in the last CTU row: the last band whatever the number of threads
    d.cu["w"][k] = 0

    def fail(threads):
        ctx = _context(stub, W, H, l2, threads)
        p = d.c()
        j = stub.vvr_submit(ctx, C.byref(p))
        rc = stub.vvr_wait(ctx, j) if j >= 0 else j
        msg = stub.vvr_last_error(ctx).decode()
        stub.vvr_destroy(ctx)
        return rc, msg
    want = fail(0)
    assert want[0] != abi.VVR_OK and want[0] < 0
    for threads in THREADS:
        assert fail(threads) == want, threads
    # (two bad records, one in the first band: that one is reported)
    d.cu["h"][2] = 0
    want2 = fail(0)
    assert want2[0] < 0
    for threads in (2, 8):
        assert fail(threads) == want2, threads
