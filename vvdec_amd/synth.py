"""Synthetic pre-parsed VVC picture stream (measurement/test infrastructure; wraps tools/synth.cpp).

`generate(params)` returns a PictureDesc; `ra_gop(...)` yields the pictures of a hierarchical-B random-access stream
 with DPB slot assignment, in decode order.
"""
import ctypes as C
import os
import subprocess
import numpy as np
from . import abi, desc

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
_SRC = os.path.join(_ROOT, "tools", "synth.cpp")
_LIB = os.path.join(_ROOT, "tools", "libvvrsynth.so")


def build(force=False):
    hdr = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vvr.h")       # (the generator writes vvr.h records and the ABI version)
    if force or not os.path.exists(_LIB) or os.path.getmtime(_LIB) < max(os.path.getmtime(_SRC), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-std=c++14", "-O2", "-fPIC", "-shared", "-Wall", _SRC, "-o", _LIB])
    return _LIB


MAX_TILE_COLS, MAX_TILE_ROWS = 20, 32                  # VVS_MAX_TILE_COLS / _ROWS
SLICES_RASTER, SLICES_RECT = 1, 2                      # Params.slice_mode
ERRORS = {-3: "a partitioning no PPS can express (tile grid / slice map)", -4: "virtual boundaries the picture header cannot carry (multiples of 8 inside the picture, ascending, one CTU apart)"}


class Params(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("width", C.c_uint16), ("height", C.c_uint16),
                ("bit_depth", C.c_uint8), ("log2_ctu", C.c_uint8), ("chroma_format", C.c_uint8), ("slice_type", C.c_uint8),
                ("tool_flags", C.c_uint32), ("num_ref", C.c_int8 * 2), ("poc", C.c_int32),
                ("ref_poc", C.c_int32 * abi.VVR_MAX_REFS * 2), ("ref_slot", C.c_int16 * abi.VVR_MAX_REFS * 2), ("out_slot", C.c_int16),
                ("base_qp", C.c_int8), ("min_cu_log2", C.c_uint8),
                ("p_intra", C.c_float), ("p_bi", C.c_float), ("p_coded", C.c_float), ("p_coded_chroma", C.c_float),
                ("p_small_corner", C.c_float), ("p_mts", C.c_float), ("p_ts", C.c_float), ("p_lfnst", C.c_float),
                ("p_split_scale", C.c_float), ("mv_sigma", C.c_float),
                ("p_sao", C.c_float), ("p_alf_luma", C.c_float), ("p_alf_chroma", C.c_float), ("p_ccalf", C.c_float),
                ("p_imv_hpel", C.c_float), ("p_jccr", C.c_float), ("p_mrl", C.c_float), ("p_bdpcm", C.c_float),
                ("p_affine", C.c_float), ("p_geo", C.c_float), ("p_ciip", C.c_float), ("p_sbtmvp", C.c_float), ("p_bcw", C.c_float), ("p_cclm", C.c_float), ("p_mip", C.c_float), ("p_sbt", C.c_float), ("p_isp", C.c_float), ("dual_tree", C.c_float), ("p_ibc", C.c_float),
                ("num_slices", C.c_uint8), ("tile_cols", C.c_uint8), ("tile_rows", C.c_uint8), ("wrap_offset", C.c_uint16), ("subpics", C.c_uint8), ("intra_slices", C.c_uint8), ("virtual_boundaries", C.c_uint8), ("scaled_refs", C.c_uint16 * 2), ("mv_window", C.c_uint16),
                ("mv_window_ver", C.c_uint16), ("p_mv_limit", C.c_float),
                ("lmcs_shape", C.c_uint8), ("min_qp_ts", C.c_uint8), ("chroma_qp_flavour", C.c_uint8), ("chroma_qp_model", C.c_uint32),
                ("tile_col_w", C.c_uint8 * (MAX_TILE_COLS + 1)), ("tile_row_h", C.c_uint8 * (MAX_TILE_ROWS + 1)), ("slice_mode", C.c_uint8),
                ("slice_map", C.c_void_p), ("slice_map_len", C.c_uint32), ("vb_x", C.c_uint16 * 4), ("vb_y", C.c_uint16 * 4), ("p_boundary_bt", C.c_float),
                ("grid_w", C.c_uint8), ("grid_h", C.c_uint8)]      # both > 0: every CTU is cut into a uniform grid of CUs of this size, no split is drawn


# Params.lmcs_shape: LMCS models at the ends of what lmcs_data() allows (tools/synth.cpp, genLmcs)
LMCS_SHAPES = {"drawn": 0, "single_bin_low": 1, "single_bin_high": 2, "late_early": 3, "sawtooth": 4, "crs_low": 5, "crs_high": 6, "nearly_identity_full": 7}
CQP_GENERAL, CQP_CLIP, CQP_LIFTED = 0, 1, 2       # Params.chroma_qp_flavour


class ChromaQpModel(C.Structure):
    """what a stream's SPS / PPS / slice header / CUs would carry about chroma QPs (tools/synth.cpp, vvs_chroma_qp): the generator fills it beside the
    description, whose TU records hold the resulting QPs; the checkers install it into the parameter sets of a reference decoder"""
    _fields_ = [("table", C.c_int8 * 76 * 3), ("pps_offset", C.c_int8 * 3), ("slice_offset", C.c_int8 * 3), ("list", C.c_int8 * 3 * 6),
                ("num_cu", C.c_uint32), ("cu_idx", C.c_void_p)]


class Buffers(C.Structure):
    _fields_ = [("cu", C.c_void_p), ("max_cu", C.c_uint32), ("tu", C.c_void_p), ("max_tu", C.c_uint32),
                ("coef", C.c_void_p), ("max_coef", C.c_uint64), ("ctu_first_cu", C.c_void_p),
                ("motion", C.c_void_p), ("lfp", C.c_void_p * 2), ("sao", C.c_void_p), ("alf", C.c_void_p), ("alf_params", C.c_void_p), ("lmcs", C.c_void_p), ("wp", C.c_void_p), ("scaling", C.c_void_p), ("ctu_slice", C.c_void_p), ("ctu_tile", C.c_void_p), ("subpics", C.c_void_p), ("cqp", C.c_void_p),
                ("num_cu", C.c_uint32), ("num_tu", C.c_uint32), ("num_coef", C.c_uint64), ("num_dmvr", C.c_uint32), ("num_subpics", C.c_uint32),
                ("hdr", abi.PicHeader)]


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.vvs_generate.restype = C.c_int
    return _lib


def default_params(**kw):
    p = Params()
    lib().vvs_default_params(C.byref(p))
    for k, v in kw.items():
        if k == "slice_map":      # (mode, per-CTU slice indices): raster_slices() / rect_slices(); the array lives as long as the parameters
            p.slice_mode, p._slice_map = v[0], np.ascontiguousarray(v[1], np.uint16)
            p.slice_map, p.slice_map_len = p._slice_map.ctypes.data, len(p._slice_map)
        elif k in ("tile_col_w", "tile_row_h", "vb_x", "vb_y"):      # zero-terminated lists
            a = getattr(p, k)
            assert len(v) <= len(a), k                # (the generator refuses a list that fills the array: no terminator)
            for i in range(len(a)):
                a[i] = v[i] if i < len(v) else 0
        else:
            setattr(p, k, v)
    return p


def tile_of_ctu(col_w, row_h):
    """tile index of every CTU (picture raster order) of the grid with these column widths / row heights in CTUs -> array [sum(row_h), sum(col_w)]"""
    col, row = np.repeat(np.arange(len(col_w)), col_w), np.repeat(np.arange(len(row_h)), row_h)
    return (row[:, None] * len(col_w) + col[None, :]).astype(np.uint16)


def raster_slices(col_w, row_h, runs):
    """Params.slice_map of raster-scan slices over a tile grid: `runs` tiles each, in tile raster order"""
    assert sum(runs) == len(col_w) * len(row_h) and min(runs) > 0
    return SLICES_RASTER, np.repeat(np.arange(len(runs)), runs).astype(np.uint16)[tile_of_ctu(col_w, row_h)].reshape(-1)


def rect_slices(col_w, row_h, tiles):
    """Params.slice_map of rectangular slices over a tile grid.  `tiles` says per tile (raster order) what becomes of it: "whole" - a slice of its own (or the first tile
    of a slice that later tiles join); a tuple of heights in CTU rows - cut into that many slices, top to bottom; ("join", k) - part of the slice tile k belongs to.
    Slices are numbered in the order their first tile comes.  The generator checks that every slice is something a PPS can express; this only numbers them"""
    t = tile_of_ctu(col_w, row_h)
    m = np.zeros(t.shape, np.uint16)
    first, n = {}, 0
    assert len(tiles) == len(col_w) * len(row_h)
    for k, what in enumerate(tiles):
        ys, xs = np.nonzero(t == k)
        if what == "whole":
            first[k], n = n, n + 1
            m[t == k] = first[k]
        elif what[0] == "join":
            first[k] = first[what[1]]
            m[t == k] = first[k]
        else:
            assert sum(what) == ys.max() - ys.min() + 1, "bands of tile %d" % k
            y = int(ys.min())
            for hgt in what:
                m[y:y + hgt, xs.min():xs.max() + 1] = n
                y, n = y + hgt, n + 1
    return SLICES_RECT, m.reshape(-1)


def set_refs(p, l0, l1=()):
    for l, lst in enumerate((l0, l1)):
        p.num_ref[l] = len(lst)
        for i, (slot, poc) in enumerate(lst):
            p.ref_slot[l][i] = slot
            p.ref_poc[l][i] = poc


def _compact(a, n, alloc=None):
    """the first n records as an array of their own, copied byte by byte (a field-wise copy would leave the padding bytes of the
    records uninitialised, and descriptions should be reproducible down to the byte)"""
    out = alloc(n, a.dtype) if alloc else np.zeros(n, a.dtype)
    out.view(np.uint8)[:] = a[:n].view(np.uint8)
    return out


def generate(p, alloc=None):
    """Run the generator; returns a desc.PictureDesc owning compact copies of all arrays (alloc: see desc.PictureDesc)."""
    L = lib()
    mcu, mtu, mcoef = C.c_uint32(), C.c_uint32(), C.c_uint64()
    L.vvs_bounds(C.byref(p), C.byref(mcu), C.byref(mtu), C.byref(mcoef))
    d = desc.PictureDesc(p.width, p.height, p.bit_depth, p.log2_ctu, p.chroma_format, p.slice_type, p.poc, p.out_slot, p.tool_flags, alloc=alloc)
    cu = np.zeros(mcu.value, desc.CU_DT)
    tu = np.zeros(mtu.value, desc.TU_DT)
    coef = np.zeros(mcoef.value, np.int16)
    d.motion = np.zeros(d.w4 * d.h4, desc.MOTION_DT)
    d.sao = np.zeros(d.num_ctu, desc.SAO_DT)
    d.alf = np.zeros(d.num_ctu, desc.ALF_DT)
    d.alf_params = abi.AlfParams()
    b = Buffers()
    b.cu, b.max_cu, b.tu, b.max_tu = cu.ctypes.data, mcu.value, tu.ctypes.data, mtu.value
    b.coef, b.max_coef = coef.ctypes.data, mcoef.value
    b.ctu_first_cu = d.ctu_first_cu.ctypes.data
    b.motion = d.motion.ctypes.data
    b.lfp[0], b.lfp[1] = d.lfp[0].ctypes.data, d.lfp[1].ctypes.data
    b.sao, b.alf = d.sao.ctypes.data, d.alf.ctypes.data
    b.alf_params = C.addressof(d.alf_params)
    if p.tool_flags & abi.TOOL_LMCS:
        d.lmcs = abi.LmcsParams()
        b.lmcs = C.addressof(d.lmcs)
    if (p.tool_flags & abi.TOOL_WP) and p.slice_type != abi.SLICE_I:
        d.wp = abi.WpParams()
        b.wp = C.addressof(d.wp)
    if p.tool_flags & abi.TOOL_SCALING_LIST:
        d.scaling = abi.ScalingList()
        b.scaling = C.addressof(d.scaling)
    if p.num_slices > 1 or p.slice_map:
        d.ctu_slice = np.zeros(d.num_ctu, np.uint16)
        b.ctu_slice = d.ctu_slice.ctypes.data
    if p.tile_cols > 1 or p.tile_rows > 1 or p.tile_col_w[0] or p.tile_row_h[0]:
        d.ctu_tile = np.zeros(d.num_ctu, np.uint16)
        b.ctu_tile = d.ctu_tile.ctypes.data
    subpics = None
    if p.subpics & 1:
        subpics = np.zeros(255, np.dtype(abi.Subpic))
        b.subpics = subpics.ctypes.data
        if d.ctu_slice is None:                      # one slice per sub-picture
            d.ctu_slice = np.zeros(d.num_ctu, np.uint16)
            b.ctu_slice = d.ctu_slice.ctypes.data
    model = cu_idx = None
    if p.chroma_qp_model and p.chroma_format:
        model, cu_idx = ChromaQpModel(), np.zeros(mcu.value, np.uint8)
        model.cu_idx = cu_idx.ctypes.data
        b.cqp = C.addressof(model)
    rc = L.vvs_generate(C.byref(p), C.byref(b))
    if rc != 0:
        raise RuntimeError("vvs_generate failed (%d)%s" % (rc, ": " + ERRORS[rc] if rc in ERRORS else ""))
    if model is not None:       # beside the description, not in it: the ABI carries TU QPs only
        model.cu_idx_array = cu_idx[:b.num_cu].copy()
        model.cu_idx = model.cu_idx_array.ctypes.data
        d.chroma_qp_model = model
    d.hdr = abi.PicHeader.from_buffer_copy(b.hdr)
    d.cu = _compact(cu, b.num_cu, alloc)
    d.tu = _compact(tu, b.num_tu, alloc)
    d.coef = _compact(coef, max(1, b.num_coef), alloc)
    d.num_dmvr = b.num_dmvr
    if subpics is not None and b.num_subpics:
        d.subpics = subpics[:b.num_subpics].copy()
    return d


def vary_slices(d, seed, alf_sets=2, wp_sets=2, intra_slices=0):
    """Give the slices of a generated multi-slice description headers of their own (vvr_slice_header): each slice draws whether it uses dependent
    quantisation, LMCS, the explicit scaling lists (of the tools the picture has), its deblocking offsets, and which ALF / weight tables it
    refers to.  The extra tables are rearrangements of the generated one (classes, alternatives and filters rolled; weights of the entries that
    are `present` changed) so every value stays in the range the syntax allows and the CUs' mc_mode stays valid.  intra_slices: the mask the
    picture was generated with (Params.intra_slices) - those slices are I slices."""
    assert d.ctu_slice is not None, "a description with more than one slice"
    rng = np.random.default_rng(seed)
    n = int(d.ctu_slice.max()) + 1
    f = int(d.hdr.tool_flags)
    sl = np.zeros(n, np.dtype(abi.SliceHeader))
    for i in range(n):
        t = f & abi.SLICE_TOOL_MASK
        for bit in (abi.TOOL_DEP_QUANT, abi.TOOL_LMCS, abi.TOOL_SCALING_LIST):
            have = bool(f & bit) or bit == abi.TOOL_DEP_QUANT
            on = have and (i == 0 or (i > 1 and rng.random() < 0.5))      # slice 0: everything the picture has, slice 1: nothing
            t = (t | bit) if on else (t & ~bit)
        if not (t & abi.TOOL_LMCS):
            t &= ~abi.TOOL_LMCS_CSCALE
        sl["tool_flags"][i] = t
        sl["deblock_beta_offset_div2"][i] = rng.integers(-6, 7, 3)
        sl["deblock_tc_offset_div2"][i] = rng.integers(-6, 7, 3)
        sl["slice_type"][i] = abi.SLICE_I if (intra_slices >> (i & 7)) & 1 else d.hdr.slice_type
        if sl["slice_type"][i] == abi.SLICE_I:
            sl["tool_flags"][i] = int(sl["tool_flags"][i]) & ~abi.TOOL_WP
        sl["alf_set"][i] = i % alf_sets if d.alf_params is not None else 0
        sl["wp_set"][i] = i % wp_sets if d.wp is not None else 0
    d.slices = sl
    if d.alf_params is not None and alf_sets > 1:
        d.alf_sets = [d.alf_params]
        for k in range(1, alf_sets):
            a = abi.AlfParams.from_buffer_copy(d.alf_params)
            for name, axes in (("luma_coeff", (0, 1)), ("luma_clip", (0, 1)), ("chroma_coeff", (0,)), ("chroma_clip", (0,)), ("ccalf_coeff", (1,))):
                v = np.ctypeslib.as_array(getattr(a, name))
                v[...] = np.roll(v, k, axis=axes)
            d.alf_sets.append(a)
    if d.wp is not None and wp_sets > 1:
        d.wp_sets = [d.wp]
        for k in range(1, wp_sets):
            w = abi.WpParams.from_buffer_copy(d.wp)
            for l in range(2):
                for i in range(abi.VVR_MAX_REFS):
                    for c in range(3):
                        e = w.e[l][i][c]
                        if e.present:
                            e.weight = int(np.clip(e.weight + (k if (i + c) & 1 else -k) * 3, (1 << w.log2_denom[1 if c else 0]) - 128, (1 << w.log2_denom[1 if c else 0]) + 127))
                            e.offset = int(np.clip(-e.offset + k, -128, 127))
            d.wp_sets.append(w)
    return d


def _alf_tables(d):
    return list(getattr(d, "alf_sets", None) or [d.alf_params])


def alf_to_limits(d, seed, clip=None):
    """Push the ALF tables of a generated description to the limits of the syntax: every luma / chroma coefficient drawn from {-128, 127}, every
    CC-ALF tap at +-64 (the largest power of two the syntax codes), and the clipping values at index 0 (1 << bit depth: no clipping) in the even
    classes / chroma alternatives and at index 3 (the tightest) in the odd ones - or, with clip = 0 or 3, at that index everywhere"""
    rng = np.random.default_rng(seed)
    bd = int(d.hdr.bit_depth)
    cv = {0: 1 << bd, 3: 1 << (bd - 7)}                       # AlfClippingValues: index 0 and index 3 (8 bit: 256, 2; 10 bit: 1024, 8)
    for a in _alf_tables(d):
        lc, lk = np.ctypeslib.as_array(a.luma_coeff), np.ctypeslib.as_array(a.luma_clip)
        lc[..., :12] = rng.choice(np.array([-128, 127], np.int16), lc[..., :12].shape)
        for c in range(abi.VVR_ALF_CLASSES):
            lk[:, c, :12] = cv[clip if clip is not None else (3 if c & 1 else 0)]
        cc, ck = np.ctypeslib.as_array(a.chroma_coeff), np.ctypeslib.as_array(a.chroma_clip)
        cc[:, :6] = rng.choice(np.array([-128, 127], np.int16), cc[:, :6].shape)
        for alt in range(abi.VVR_ALF_MAX_CHR_ALT):
            ck[alt, :6] = cv[clip if clip is not None else (3 if alt & 1 else 0)]
        x = np.ctypeslib.as_array(a.ccalf_coeff)
        x[..., :abi.VVR_CCALF_TAPS] = rng.choice(np.array([-64, 64], np.int16), x[..., :abi.VVR_CCALF_TAPS].shape)
    return d


def wp_to_limits(d, seed):
    """Push the explicit prediction weights of a generated description to the limits of pred_weight_table(): the denominators from {0, 7} (luma and chroma
    differ), the weight of every entry that is `present` at ( 1 << denominator ) - 128 or + 127, its offset at -128 or 127.  `present` is left as generated,
    so the CUs' mc_mode and the BDOF / DMVR conditions stay valid"""
    rng = np.random.default_rng(seed)
    for k, w in enumerate(list(getattr(d, "wp_sets", None) or [d.wp])):
        w.log2_denom[0] = 7 if (seed + k) & 1 else 0
        w.log2_denom[1] = 7 - w.log2_denom[0]
        for l in range(2):
            for i in range(abi.VVR_MAX_REFS):
                for c in range(3):
                    e = w.e[l][i][c]
                    den = w.log2_denom[1 if c else 0]
                    if e.present:
                        e.weight = (1 << den) + (127 if rng.integers(2) else -128)
                        e.offset = 127 if rng.integers(2) else -128
                    else:
                        e.weight, e.offset = 1 << den, 0
    return d


def deblock_offsets_to_limits(d, sign):
    """pps / ph / sh _beta_offset_div2 and _tc_offset_div2 of every component at +6 (sign > 0) or -6: the ends of the syntax range (+-12 once doubled), in the
    picture header and in the slice headers.  (The edge tables of a description hold QPs, boundary strengths and filter lengths only: nothing to regenerate.)"""
    v = 6 if sign > 0 else -6
    for c in range(3):
        d.hdr.deblock_beta_offset_div2[c] = v
        d.hdr.deblock_tc_offset_div2[c] = v
    if getattr(d, "slices", None) is not None:
        d.slices["deblock_beta_offset_div2"][...] = v
        d.slices["deblock_tc_offset_div2"][...] = v
    return d


def rewrite_qp(d, qps):
    """Give the CUs of a generated single-tree description the luma QPs `qps` (one per CU, -QpBdOffset .. 63) and keep everything that follows from them
    consistent, the way the generator derives it: TU.qp (luma: QP + QpBdOffset; chroma: identity mapping of the QP clipped to -QpBdOffset .. 63) and the QPs of
    the edge tables (rounded mean of the two sides, LoopFilter.cpp:1363 / 1180)"""
    qps = np.asarray(qps, np.int32)
    assert len(qps) == len(d.cu) and not (d.cu["tree"] == abi.TREE_CHROMA).any(), "one QP per CU of a single-tree picture"
    assert getattr(d, "chroma_qp_model", None) is None, "identity chroma QP mapping only (the edge tables of a model are the generator's)"
    qpbd = 6 * (int(d.hdr.bit_depth) - 8)
    assert qps.min() >= -qpbd and qps.max() <= 63
    d.cu["qp"] = qps
    t = qps[d.tu["cu"]]
    d.tu["qp"][:, 0] = t + qpbd
    d.tu["qp"][:, 1] = d.tu["qp"][:, 2] = np.clip(t, -qpbd, 63) + qpbd
    q4 = np.zeros((d.h4, d.w4), np.int32)
    for cu, q in zip(d.cu, qps):
        q4[int(cu["y"]) >> 2:(int(cu["y"]) + int(cu["h"]) + 3) >> 2, int(cu["x"]) >> 2:(int(cu["x"]) + int(cu["w"]) + 3) >> 2] = q
    for dr in range(2):
        p4 = np.roll(q4, 1, axis=1 - dr)                      # the P side: the unit to the left (vertical edges) / above (horizontal edges)
        mean = ((q4 + p4 + 1) >> 1).astype(np.int8)
        valid = np.ones_like(q4, bool)
        if dr == 0:
            valid[:, 0] = False
        else:
            valid[0, :] = False
        lq = d.lfp[dr]["qp"].reshape(d.h4, d.w4, 3)
        for c in range(3):
            lq[:, :, c][valid] = mean[valid]
    return d


def model_chroma_qps(d, model=None):
    """TU.qp[1..2] restated from a chroma QP model the way QpParam derives them (Quant.cpp:65-91) -> (per TU [Cb, Cr] with each component's own table,
    per TU the QP of the joint table): a joint_cbcr == 3 TU holds the joint QP in both components, every other TU the components' own"""
    m = model or d.chroma_qp_model
    qpbd = 6 * (int(d.hdr.bit_depth) - 8)
    table = np.ctypeslib.as_array(m.table).astype(np.int32)
    tot = np.array([m.pps_offset[t] + m.slice_offset[t] for t in range(3)], np.int32)
    lst = np.concatenate([np.zeros((1, 3), np.int32), np.ctypeslib.as_array(m.list).astype(np.int32)])
    cu = d.tu["cu"].astype(np.int64)
    qpi = np.clip(d.cu["qp"].astype(np.int32)[cu], -qpbd, 63)
    idx = m.cu_idx_array[cu]
    q = np.stack([np.clip(table[t][qpi + qpbd] + tot[t] + lst[idx, t] + qpbd, 0, 63 + qpbd) for t in range(3)], axis=1)
    return q[:, :2], q[:, 2]


def attach_rpr(d, refs, win=(0, 0), colloc=(1, 1)):
    """Reference picture resampling: give a generated description its vvr_rpr_params.  refs: {(list, idx): dict(ratio=(rx, ry), size=(w, h), win=(left, top))}
    names the scaled reference pictures (the description must have been generated with Params.scaled_refs naming the same ones); every other reference
    picture of the lists has the current picture's size and window.  win: the current picture's scaling window offsets (luma samples);
    colloc: sps_chroma_horizontal / vertical_collocated_flag of the reference pictures' SPS."""
    r = abi.RprParams()
    r.win_left, r.win_top = win
    for l in range(2):
        for i in range(d.hdr.num_ref[l]):
            e = r.ref[l][i]
            spec = refs.get((l, i))
            e.ratio[0], e.ratio[1] = spec["ratio"] if spec else (1 << 14, 1 << 14)
            e.width, e.height = spec.get("size", (d.hdr.width, d.hdr.height)) if spec else (d.hdr.width, d.hdr.height)
            e.win_left, e.win_top = spec.get("win", win) if spec else win
            e.scaled = 1 if spec else 0
            e.hor_collocated_chroma, e.ver_collocated_chroma = colloc
    d.rpr = r
    return d


def picture_for_plan(plan, width, height, seed=1234, tool_flags=0, alloc=None, **kw):
    """PictureDesc of one stream.PicPlan (generator seed = base seed + POC)."""
    p = default_params(width=width, height=height, seed=seed + plan.poc, tool_flags=tool_flags, slice_type=plan.slice_type, **kw)
    p.poc = plan.poc
    p.out_slot = plan.slot
    if plan.slice_type != abi.SLICE_I:
        set_refs(p, plan.ref_slots[0], plan.ref_slots[1])
    return generate(p, alloc)


def natural_picture(width, height, seed, bit_depth=10):
    """A smooth-plus-texture test picture (stands in for an IRAP picture until intra reconstruction is enabled)."""
    rng = np.random.default_rng(seed)
    mx = (1 << bit_depth) - 1
    gy, gx = np.mgrid[0:height, 0:width]
    base = (np.sin(gx / 37.0 + seed) + np.cos(gy / 23.0 - seed) + np.sin((gx + gy) / 61.0)) * (mx / 8.0) + mx / 2.0
    blocks = rng.integers(-mx // 10, mx // 10, (height // 16 + 1, width // 16 + 1)).repeat(16, 0).repeat(16, 1)[:height, :width]
    y = np.clip(base + blocks + rng.integers(-12, 13, (height, width)), 0, mx).astype(np.uint16)
    cb = np.clip(y[::2, ::2].astype(np.int32) // 2 + mx // 4 + rng.integers(-6, 7, (height // 2, width // 2)), 0, mx).astype(np.uint16)
    cr = np.clip(mx - y[::2, ::2].astype(np.int32) // 2 - mx // 4 + rng.integers(-6, 7, (height // 2, width // 2)), 0, mx).astype(np.uint16)
    return [y, cb, cr]


EXTREME_KINDS = ("checker", "steps", "flat_max", "flat_zero", "noise", "taps")


def extreme_picture(width, height, seed, bit_depth=10, kind="checker"):
    """A test picture at the ends of the sample range, [y, cb, cr] like natural_picture; every plane follows the rule of its kind with draws of its own
    (chroma is never derived from luma).
      checker    0 / max alternating from sample to sample; phase and orientation (per sample, per row, per column) drawn anew for every 16x16 block, so
                 that fractional MVs see every alignment
      steps      0 / max blocks of 4, 8 or 16 samples, the size and a shift of 0 or 4 samples drawn per 64x64 region: edges on and off the 8-sample grid
      flat_max, flat_zero
      noise      uniform over the whole range, 0 and max present in every plane
      taps       max where the eight-tap interpolation filters are positive, 0 where they are negative (- + - + + - + - along a row, the rows that meet
                 negative taps of the second stage inverted), shifted and inverted per 32x32 block: where an MV lines up with a block, both filter stages
                 reach their largest over- and undershoot - more than on a checker, which the two centre taps see as + -"""
    assert kind in EXTREME_KINDS, kind
    rng = np.random.default_rng([seed, EXTREME_KINDS.index(kind)])
    mx = (1 << bit_depth) - 1
    out = []
    for (h, w) in ((height, width), (height // 2, width // 2), (height // 2, width // 2)):
        gy, gx = np.mgrid[0:h, 0:w]
        if kind == "checker":
            shape = (h // 16 + 1, w // 16 + 1)
            up = lambda a: a.repeat(16, 0).repeat(16, 1)[:h, :w]
            phase, orient = up(rng.integers(0, 2, shape)), up(rng.integers(0, 3, shape))
            bit = (np.where(orient == 0, gx + gy, np.where(orient == 1, gy, gx)) + phase) & 1
        elif kind == "steps":
            shape = (h // 64 + 1, w // 64 + 1)
            up = lambda a: a.repeat(64, 0).repeat(64, 1)[:h, :w]
            l2, sx, sy, phase = up(rng.integers(2, 5, shape)), up(rng.integers(0, 2, shape)) * 4, up(rng.integers(0, 2, shape)) * 4, up(rng.integers(0, 2, shape))
            bit = (((gx + sx) >> l2) + ((gy + sy) >> l2) + phase) & 1
        elif kind == "taps":
            shape = (h // 32 + 1, w // 32 + 1)
            up = lambda a: a.repeat(32, 0).repeat(32, 1)[:h, :w]
            sign = np.array([0, 1, 0, 1, 1, 0, 1, 0])
            sx, sy, phase = up(rng.integers(0, 8, shape)), up(rng.integers(0, 8, shape)), up(rng.integers(0, 2, shape))
            bit = sign[(gx + sx) & 7] ^ sign[(gy + sy) & 7] ^ phase
        elif kind == "noise":
            a = rng.integers(0, mx + 1, (h, w))
            a[0, 0], a[-1, -1] = 0, mx
            out.append(a.astype(np.uint16))
            continue
        else:
            bit = np.full((h, w), 1 if kind == "flat_max" else 0)
        out.append((bit * mx).astype(np.uint16))
    return out


def random_partition(rnd, W, H, log2_ctu, subpics_ok=True):
    """A random picture partitioning for the randomised test legs -> (tool flags to add, generator parameters).  `rnd`: a random.Random of the caller's, kept apart
    from the one that draws the rest of the picture.  Half of the draws use the generator's own layouts (num_slices / tile_cols / tile_rows / virtual_boundaries /
    subpics), half the explicit ones: a random tile grid (up to 20 columns), raster-scan slices of random runs or rectangular slices (a tile whole, cut into bands
    of CTU rows, or joined with the tile to its left), virtual boundaries at random legal positions (multiples of 8, one CTU apart)"""
    S = 1 << log2_ctu
    cx, cy = (W + S - 1) >> log2_ctu, (H + S - 1) >> log2_ctu
    tools = (abi.TOOL_NO_LF_ACROSS_SLICES if rnd.random() < 0.5 else 0) | (abi.TOOL_NO_LF_ACROSS_TILES if rnd.random() < 0.5 else 0)
    kw = {}
    if rnd.random() < 0.5:
        if rnd.random() < 0.7:
            kw["tile_cols"], kw["tile_rows"] = rnd.randrange(1, 4), rnd.randrange(1, 4)
        if rnd.random() < 0.6:
            kw["num_slices"] = rnd.randrange(2, 6)
        if rnd.random() < 0.5:
            # (at most two per direction: the drawn positions ignore the one-CTU spacing, and three that touch one CTU are more than the reference's filters take)
            kw["virtual_boundaries"] = rnd.randrange(3) | (rnd.randrange(3) << 2) | (16 if rnd.random() < 0.5 else 0)
        if subpics_ok and rnd.random() < 0.25 and kw.get("tile_cols", 1) * kw.get("tile_rows", 1) > 1:
            kw["subpics"] = 1 | (rnd.randrange(3) << 1) | (rnd.randrange(3) << 3)
        return tools, kw

    def cut(n, most):
        parts = []
        while n:
            parts.append(rnd.randrange(1, n + 1) if len(parts) + 1 < most else n)
            if rnd.random() < 0.5:
                parts[-1] = min(parts[-1], 1 + rnd.randrange(2))
            n -= parts[-1]
        return tuple(parts)
    cols, rows = cut(cx, MAX_TILE_COLS), cut(cy, MAX_TILE_ROWS)
    kw["tile_col_w"], kw["tile_row_h"] = cols, rows
    nt = len(cols) * len(rows)
    how = rnd.randrange(4)
    if how == 0 and subpics_ok and 1 < nt <= 255:
        kw["subpics"] = 1 | (rnd.randrange(3) << 1) | (rnd.randrange(3) << 3)
    elif how == 1 and nt > 1:
        runs = []
        while sum(runs) < nt:
            runs.append(rnd.randrange(1, min(nt - sum(runs), 2 * len(cols)) + 1))
        if len(runs) > 1:
            kw["slice_map"] = raster_slices(cols, rows, runs)
    elif how == 2:
        tiles = []
        for k in range(nt):
            hgt = rows[k // len(cols)]
            r = rnd.random()
            if r < 0.3 and k % len(cols) and (tiles[k - 1] == "whole" or tiles[k - 1][0] == "join"):       # (a run of tiles inside one tile row: a rectangle)
                tiles.append(("join", k - 1))
            elif r < 0.6 and hgt > 1:
                bands = cut(hgt, hgt)
                tiles.append(bands if len(bands) > 1 else "whole")
            else:
                tiles.append("whole")
        mode, m = rect_slices(cols, rows, tiles)
        if m.max() > 0:
            kw["slice_map"] = (mode, m)
    for name, lim in (("vb_x", W), ("vb_y", H)):
        pos, v = [], 8 * rnd.randrange(1, max(2, lim // 8))
        for _ in range(rnd.randrange(4)):
            if v >= lim:
                break
            pos.append(v)
            v += S + 8 * rnd.randrange(0, max(1, lim // 16))
        if pos and rnd.random() < 0.6:
            kw[name] = tuple(pos)
    return tools, kw
