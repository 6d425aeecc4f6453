"""ctypes mirror of include/vvr.h (the C ABI of the reconstruction back-end).

Field names, order and widths follow include/vvr.h one to one; `tests/test_abi.py` checks sizeof/offsetof against the
compiled library so the two cannot drift apart silently.
"""
import ctypes as C
import math

VVR_ABI_VERSION = 5
VVR_MAX_REFS = 16
VVR_MAX_ALF_APS = 8
VVR_ALF_CLASSES = 25
VVR_ALF_LUMA_TAPS = 13
VVR_ALF_CHR_TAPS = 7
VVR_ALF_MAX_CHR_ALT = 8
VVR_CCALF_FILTERS = 4
VVR_CCALF_TAPS = 7

# status codes
VVR_OK, VVR_ERR_UNSPECIFIED, VVR_ERR_PARAMETER, VVR_ERR_UNSUPPORTED, VVR_ERR_DEVICE, VVR_ERR_NO_DEVICE, VVR_ERR_BUSY = 0, -1, -2, -3, -4, -5, -6
VVR_NOT_READY = 1          # non-blocking stream-order queries: ask again

# tool flags
TOOL_SAO_LUMA, TOOL_SAO_CHROMA, TOOL_ALF, TOOL_CCALF, TOOL_LMCS, TOOL_LMCS_CSCALE, TOOL_DEBLOCK_OFF, TOOL_DEP_QUANT, \
    TOOL_BDOF, TOOL_DMVR, TOOL_PROF, TOOL_JCCR_SIGN, TOOL_STILL_REF, TOOL_LFNST, TOOL_MTS, TOOL_CCLM_COLLOC, \
    TOOL_WP, TOOL_SCALING_LIST, TOOL_SCALING_LIST_NO_LFNST, TOOL_IMPLICIT_MTS, TOOL_IBC, TOOL_LADF, TOOL_NO_LF_ACROSS_SLICES, TOOL_NO_LF_ACROSS_TILES, TOOL_AFFINE_MV_ON_DEVICE, TOOL_COL_MOTION, TOOL_LFP_ON_DEVICE = [1 << i for i in range(27)]
SLICE_TOOL_MASK = TOOL_DEP_QUANT | TOOL_LMCS | TOOL_LMCS_CSCALE | TOOL_SCALING_LIST | TOOL_WP       # VVR_SLICE_TOOL_MASK: the switches a vvr_slice_header carries

PRED_INTER, PRED_INTRA, PRED_IBC = 0, 1, 2
TREE_JOINT, TREE_LUMA, TREE_CHROMA = 0, 1, 2
CU_ROOT_CBF, CU_SKIP, CU_MERGE, CU_AFFINE, CU_AFFINE_6P, CU_CIIP, CU_GEO, CU_SBTMVP, CU_MIP, CU_MIP_TRANSP, CU_SMVD, CU_MMVD = [1 << i for i in range(12)]
MC_NONE, MC_UNI, MC_BI, MC_BDOF, MC_DMVR, MC_DMVR_BDOF, MC_AFFINE, MC_SBTMVP, MC_GEO = range(9)
MTS_DCT2, MTS_SKIP, MTS_DST7_DST7, MTS_DCT8_DST7, MTS_DST7_DCT8, MTS_DCT8_DCT8 = range(6)
TR_DCT2, TR_DCT8, TR_DST7 = 0, 1, 2
SLICE_B, SLICE_P, SLICE_I = 0, 1, 2
STOP_NONE, STOP_RECO, STOP_DEBLOCK, STOP_SAO = 0, 1, 2, 3

u8, i8, u16, i16, u32, i32, u64 = C.c_uint8, C.c_int8, C.c_uint16, C.c_int16, C.c_uint32, C.c_int32, C.c_uint64


class AlfParams(C.Structure):
    _fields_ = [("luma_coeff", i16 * VVR_ALF_LUMA_TAPS * VVR_ALF_CLASSES * VVR_MAX_ALF_APS),
                ("luma_clip", i16 * VVR_ALF_LUMA_TAPS * VVR_ALF_CLASSES * VVR_MAX_ALF_APS),
                ("chroma_coeff", i16 * VVR_ALF_CHR_TAPS * VVR_ALF_MAX_CHR_ALT),
                ("chroma_clip", i16 * VVR_ALF_CHR_TAPS * VVR_ALF_MAX_CHR_ALT),
                ("ccalf_coeff", i16 * (VVR_CCALF_TAPS + 1) * VVR_CCALF_FILTERS * 2),
                ("num_luma_aps", u8), ("pad", u8 * 7)]


class LmcsParams(C.Structure):
    _fields_ = [("fwd_lut", i16 * 4096), ("inv_lut", i16 * 4096), ("chroma_scale", i16 * 16), ("pivot", i16 * 17), ("min_bin", i16), ("max_bin", i16),
                ("model_delta_cw", i16 * 16), ("model_delta_crs", i16), ("pad", i16 * 4)]


class PicHeader(C.Structure):
    _fields_ = [("abi_version", u32), ("tool_flags", u32), ("width", u16), ("height", u16),
                ("chroma_format", u8), ("bit_depth", u8), ("log2_ctu", u8), ("slice_type", u8),
                ("poc", i32), ("out_slot", i16), ("num_ref", i8 * 2),
                ("ref_slot", i16 * VVR_MAX_REFS * 2), ("ref_poc", i32 * VVR_MAX_REFS * 2),
                ("deblock_beta_offset_div2", i8 * 3), ("deblock_tc_offset_div2", i8 * 3),
                ("log2_sao_offset_scale", u8 * 2), ("min_qp_ts", i8),
                ("ladf_num_intervals", u8), ("ladf_qp_offset", i8 * 5), ("pad", u8), ("ladf_lower_bound", i16 * 5),
                ("num_ver_vb", u8), ("num_hor_vb", u8), ("wrap_offset", u16), ("pad2", u8 * 2), ("vb_pos_x", u16 * 3), ("vb_pos_y", u16 * 3), ("pad3", u8 * 4)]


class Cu(C.Structure):
    _fields_ = [("x", u16), ("y", u16), ("w", u8), ("h", u8), ("tree", u8), ("pred_mode", u8),
                ("flags", u16), ("qp", i8), ("mc_mode", u8),
                ("intra_dir", u8 * 2), ("multi_ref_idx", u8), ("isp_mode", u8), ("bdpcm", u8 * 2), ("lfnst_idx", u8), ("sbt_info", u8),
                ("inter_dir", u8), ("ref_idx", i8 * 2), ("bcw_idx", u8), ("imv", u8), ("geo_split_dir", u8), ("geo_dir_ref", u8 * 2),
                ("ciip_neigh_intra", u8), ("lfnst_intra_mode", u8), ("pad0", u8 * 2),
                ("mv", i32 * 2 * 3 * 2), ("geo_mv", i32 * 2 * 2),
                ("first_tu", u32), ("num_tu", u32), ("dmvr_off", u32), ("pad1", u32)]


class Tu(C.Structure):
    _fields_ = [("x", u16), ("y", u16), ("w", u8), ("h", u8), ("comp_mask", u8), ("cbf", u8), ("joint_cbcr", u8),
                ("mts_idx", u8 * 3), ("max_scan_x", u8 * 3), ("max_scan_y", u8 * 3), ("qp", i8 * 3), ("tr_type", u8 * 3), ("pad0", u8),
                ("coef_off", u32 * 3), ("cu", u32)]


class Motion(C.Structure):
    _fields_ = [("mv", i32 * 2 * 2), ("ref_idx", i8 * 2), ("pad", u8 * 2)]


class Lfp(C.Structure):
    _fields_ = [("qp", i8 * 3), ("bs", u8), ("side_max_filt_length", u8), ("flags", u8), ("pad", u8 * 2)]


class SaoCtu(C.Structure):
    _fields_ = [("mode", u8 * 3), ("type", u8 * 3), ("band_pos", u8 * 3), ("offset", i8 * 4 * 3), ("pad", u8 * 3)]


class AlfCtu(C.Structure):
    _fields_ = [("cc_idc", u8 * 2), ("enable", u8 * 3), ("alt", u8 * 2), ("pad", u8), ("luma_filter_idx", i16), ("pad2", u8 * 2)]


class WpEntry(C.Structure):
    _fields_ = [("weight", i16), ("offset", i16), ("present", u8), ("pad", u8 * 3)]


class WpParams(C.Structure):
    _fields_ = [("log2_denom", u8 * 2), ("pad", u8 * 6), ("e", WpEntry * 3 * VVR_MAX_REFS * 2)]


class ScalingList(C.Structure):
    _fields_ = [("coef", u8 * 64 * 28), ("dc", u8 * 28), ("pad", u8 * 4)]


class Subpic(C.Structure):
    _fields_ = [("x0", u16), ("y0", u16), ("x1", u16), ("y1", u16), ("treated_as_pic", u8), ("lf_across", u8), ("pad", u8 * 2)]


class SliceHeader(C.Structure):      # vvr_slice_header: what a slice header sets for its slice only
    _fields_ = [("tool_flags", u32), ("deblock_beta_offset_div2", i8 * 3), ("deblock_tc_offset_div2", i8 * 3), ("slice_type", u8), ("alf_set", u8), ("wp_set", u8), ("pad", u8 * 3)]


class RprRef(C.Structure):           # vvr_rpr_ref: one reference picture as the current picture sees it (reference picture resampling)
    _fields_ = [("ratio", i32 * 2), ("win_left", i32), ("win_top", i32), ("width", u16), ("height", u16), ("scaled", u8), ("hor_collocated_chroma", u8), ("ver_collocated_chroma", u8), ("pad", u8)]


class RprParams(C.Structure):
    _fields_ = [("win_left", i32), ("win_top", i32), ("ref", RprRef * VVR_MAX_REFS * 2)]


class Picture(C.Structure):
    _fields_ = [("hdr", PicHeader), ("num_cu", u32), ("num_tu", u32),
                ("cu", C.POINTER(Cu)), ("tu", C.POINTER(Tu)), ("ctu_first_cu", C.POINTER(u32)),
                ("coef", C.POINTER(i16)), ("num_coef", u64),
                ("motion", C.POINTER(Motion)), ("lfp", C.POINTER(Lfp) * 2),
                ("sao", C.POINTER(SaoCtu)), ("alf", C.POINTER(AlfCtu)),
                ("alf_params", C.POINTER(AlfParams)), ("lmcs", C.POINTER(LmcsParams)),
                ("wp", C.POINTER(WpParams)), ("scaling", C.POINTER(ScalingList)),
                ("ctu_slice", C.POINTER(u16)), ("ctu_tile", C.POINTER(u16)), ("subpics", C.c_void_p), ("num_subpics", u32),
                ("slices", C.POINTER(SliceHeader)), ("rpr", C.POINTER(RprParams)), ("num_slices", u32), ("num_alf_sets", u32), ("num_wp_sets", u32), ("resident", C.c_int)]


class Config(C.Structure):
    _fields_ = [("abi_version", u32), ("device", i32), ("max_width", u16), ("max_height", u16),
                ("chroma_format", u8), ("bit_depth", u8), ("log2_ctu", u8), ("num_slots", u8), ("num_streams", u8), ("host_threads", u8), ("stop_after", u8), ("ring_entries", u8),
                ("read_buffers", u8), ("pad", u8 * 7), ("ext_planes", C.c_void_p)]


class FilmGrainBank(C.Structure):
    """vvr_film_grain_bank: the film grain model's state after the reference's FilmGrain::updateFGC (vvr.h)"""
    _fields_ = [("struct_size", u32), ("comp_present", u8 * 3), ("shift", u8), ("scale_lut", (u8 * 256) * 3), ("pattern_lut", (u8 * 256) * 3),
                ("pattern", (((C.c_int8 * 64) * 64) * 8) * 2)]


def film_grain_bank(comp_present, shift, scale_lut, pattern_lut, pattern):
    """a FilmGrainBank from its fields as arrays: comp_present (3,), shift, scale_lut and pattern_lut (3, 256) uint8, pattern (2, 8, 64, 64) int8"""
    import numpy as np
    b = FilmGrainBank()
    b.struct_size = C.sizeof(FilmGrainBank)
    b.shift = int(shift)
    for name, arr, dt in (("comp_present", comp_present, np.uint8), ("scale_lut", scale_lut, np.uint8), ("pattern_lut", pattern_lut, np.uint8), ("pattern", pattern, np.int8)):
        field = getattr(b, name)
        a = np.ascontiguousarray(arr, dtype=dt)
        assert a.nbytes == C.sizeof(field), name
        C.memmove(C.addressof(field), a.ctypes.data, a.nbytes)
    return b


OUT_PLANAR16, OUT_PLANAR8, OUT_PACKED10, OUT_NV12, OUT_P010, OUT_RGB8, OUT_RGB16, OUT_RGBF16 = 0, 1, 2, 16, 17, 32, 33, 34
OUT_RGBF32, OUT_RGBA8, OUT_BGRA8, OUT_RGB24, OUT_BGR24, OUT_RGB10A2, OUT_RGBA16F = 36, 48, 49, 50, 51, 52, 53
OUT_YUV444P8, OUT_YUV444P16, OUT_YUV422P8, OUT_YUV422P16, OUT_UYVY, OUT_YUY2, OUT_Y210, OUT_V210, OUT_Y410 = 64, 65, 66, 67, 68, 69, 70, 71, 72
OUT_FORMATS = {"planar16": OUT_PLANAR16, "planar8": OUT_PLANAR8, "packed10": OUT_PACKED10, "nv12": OUT_NV12, "p010": OUT_P010,
               "rgb8": OUT_RGB8, "rgb16": OUT_RGB16, "rgbf16": OUT_RGBF16, "rgbf32": OUT_RGBF32, "rgba8": OUT_RGBA8, "bgra8": OUT_BGRA8,
               "rgb24": OUT_RGB24, "bgr24": OUT_BGR24, "rgb10a2": OUT_RGB10A2, "rgba16f": OUT_RGBA16F,
               "yuv444p8": OUT_YUV444P8, "yuv444p16": OUT_YUV444P16, "yuv422p8": OUT_YUV422P8, "yuv422p16": OUT_YUV422P16, "uyvy": OUT_UYVY, "yuy2": OUT_YUY2,
               "y210": OUT_Y210, "v210": OUT_V210, "y410": OUT_Y410}
# Y'CbCr at 4:4:4 / 4:2:2: the packed formats are one plane, elements of the plane's dtype per row as a function of the width
OUT_YUV_PACKED = {"uyvy": lambda w: 2 * w, "yuy2": lambda w: 2 * w, "y210": lambda w: 2 * w, "v210": lambda w: (w + 5) // 6 * 4, "y410": lambda w: w}
# the interleaved formats: elements of the plane's dtype per pixel (rgb10a2: one uint32)
OUT_INTERLEAVED = {"rgba8": 4, "bgra8": 4, "rgb24": 3, "bgr24": 3, "rgba16f": 4, "rgb10a2": 1}
# vvr_set_output_narrowing: how the byte-per-sample Y'CbCr formats leave a context of 9 or 10 bits (VVR_NARROW_*); OUT_NARROWED: the formats it is looked at for
NARROW_REFUSE, NARROW_TRUNCATE, NARROW_ROUND, NARROW_DITHER = 0, 1, 2, 3
NARROW_MODES = {"refuse": NARROW_REFUSE, "truncate": NARROW_TRUNCATE, "round": NARROW_ROUND, "dither": NARROW_DITHER}
OUT_NARROWED = ("planar8", "nv12", "yuv444p8", "yuv422p8", "uyvy", "yuy2")


# vvr_set_output_resampling: the filter out_w / out_h resample with (VVR_RESAMPLE_*); None / "reference": the reference's DCTIF
RESAMPLE_REFERENCE, RESAMPLE_AREA, RESAMPLE_TRIANGLE, RESAMPLE_CUBIC = 0, 1, 2, 3
RESAMPLE_FILTERS = {None: RESAMPLE_REFERENCE, "reference": RESAMPLE_REFERENCE, "area": RESAMPLE_AREA, "triangle": RESAMPLE_TRIANGLE, "cubic": RESAMPLE_CUBIC}
RESAMPLE_MAX_TAPS = 256


def resample_taps(L, filter, n, m, phase, i):
    """vvr_resample_taps: (first, [weights]) of output sample i of an axis of n source and m output samples (phase: 2, or 1 for chroma that is
    collocated on the axis), or None where the call refuses.  filter: 1 .. 3 or a name of RESAMPLE_FILTERS"""
    first, w = C.c_int32(0), (C.c_int16 * RESAMPLE_MAX_TAPS)()
    count = L.vvr_resample_taps(RESAMPLE_FILTERS.get(filter, filter), int(n), int(m), int(phase), int(i), C.byref(first), w)
    return None if count < 0 else (first.value, list(w[:count]))


class OutputRequest(C.Structure):
    """vvr_output_request: one request of the output queue (vvr_output_submit, vvr.h)"""
    _fields_ = [("struct_size", u32), ("slot", i32), ("job", i32), ("x", i32), ("y", i32), ("w", i32), ("h", i32), ("out_w", i32), ("out_h", i32),
                ("collocated", u8), ("format", u8), ("grain", u8), ("blocking", u8), ("dst", C.c_void_p * 3), ("dst_stride_bytes", C.c_size_t * 3)]


def output_request(slot, job, window, fmt, size, collocated, grain, blocking, planes):
    """an OutputRequest whose destinations are `planes` (rows at their strides): numpy arrays, or 2-D torch tensors on the context's device"""
    r = OutputRequest()
    r.struct_size = C.sizeof(OutputRequest)
    r.slot, r.job = slot, -1 if job is None else job
    r.x, r.y, r.w, r.h = window
    r.out_w, r.out_h = size or (0, 0)
    r.collocated = int(bool(collocated[0])) | int(bool(collocated[1])) << 1
    r.format, r.grain, r.blocking = OUT_FORMATS[fmt] if isinstance(fmt, str) else fmt, 1 if grain else 0, 1 if blocking else 0
    for c, a in enumerate(planes):
        if hasattr(a, "data_ptr"):
            r.dst[c], r.dst_stride_bytes[c] = a.data_ptr(), a.stride(0) * a.element_size()
        else:
            r.dst[c], r.dst_stride_bytes[c] = a.ctypes.data, a.strides[0]
    return r


OUT_BATCH_MAX = 256
OUT_BATCH_FORMATS = ("rgb8", "rgb16", "rgbf16", "rgbf32", "rgba8", "bgra8", "rgb24", "bgr24", "rgb10a2", "rgba16f")


class OutputBatch(C.Structure):
    """vvr_output_batch: the regions of a batch request (vvr_output_submit_batch, vvr.h)"""
    _fields_ = [("struct_size", u32), ("count", u32), ("origin", C.POINTER(i32)), ("batch_stride_bytes", C.c_size_t * 3)]


def output_batch(origins, batch_stride_bytes):
    """an OutputBatch of the regions at `origins` ((x, y) pairs) whose planes lie batch_stride_bytes[k] apart -> (the struct, the array it
    points to: keep it until the call has returned)"""
    flat = [int(v) for o in origins for v in o]
    arr = (i32 * max(1, len(flat)))(*flat)
    b = OutputBatch()
    b.struct_size, b.count, b.origin = C.sizeof(OutputBatch), len(flat) // 2, C.cast(arr, C.POINTER(i32))
    for k, v in enumerate(batch_stride_bytes):
        b.batch_stride_bytes[k] = int(v)
    return b, arr


def output_plane_shapes(window, fmt, size, ncomp):
    """(rows, bytes or samples per row) of every plane a request produces, and the dtype: packed10 rows are w / 4 * 5 bytes; the semi-planar
    formats have two planes, luma and the interleaved CbCr rows of 2 * (w >> 1) samples (nv12: uint8, p010: uint16); the RGB formats three
    planes at the luma size (rgb8: uint8, rgb16: uint16, rgbf16: float16, rgbf32: float32); the interleaved formats one plane of (h, w * C)
    uint8 (rgba8, bgra8: C = 4; rgb24, bgr24: C = 3) or float16 (rgba16f: C = 4), rgb10a2 one plane of (h, w) uint32; Y'CbCr at 4:4:4 three planes
    at the luma size (yuv444p8: uint8, yuv444p16: uint16), at 4:2:2 Y (h, w) and Cb, Cr (h, w >> 1) (yuv422p8, yuv422p16), or one packed plane:
    uyvy, yuy2 (h, 2 w) uint8, y210 (h, 2 w) uint16, v210 (h, (w + 5) // 6 * 4) uint32 - six pixels in four dwords - and y410 (h, w) uint32"""
    import numpy as np
    w, h = size or (window[2], window[3])
    if fmt in ("rgb8", "rgb16", "rgbf16", "rgbf32"):
        return [(h, w)] * 3, {"rgb8": np.uint8, "rgb16": np.uint16, "rgbf16": np.float16, "rgbf32": np.float32}[fmt]
    if fmt in ("yuv444p8", "yuv444p16"):
        return [(h, w)] * 3, np.uint8 if fmt == "yuv444p8" else np.uint16
    if fmt in ("yuv422p8", "yuv422p16"):
        return [(h, w), (h, w >> 1), (h, w >> 1)], np.uint8 if fmt == "yuv422p8" else np.uint16
    if fmt in OUT_YUV_PACKED:
        return [(h, OUT_YUV_PACKED[fmt](w))], np.uint8 if fmt in ("uyvy", "yuy2") else np.uint16 if fmt == "y210" else np.uint32
    if fmt in OUT_INTERLEAVED:
        return [(h, w * OUT_INTERLEAVED[fmt])], np.uint32 if fmt == "rgb10a2" else np.float16 if fmt == "rgba16f" else np.uint8
    shapes = [(h >> (1 if c else 0), w >> (1 if c else 0)) for c in range(ncomp)]
    if fmt in ("nv12", "p010"):
        return [(h, w), (h >> 1, 2 * (w >> 1))], np.uint8 if fmt == "nv12" else np.uint16
    if fmt == "packed10":
        return [(r, n // 4 * 5) for r, n in shapes], np.uint8
    return shapes, np.uint8 if fmt == "planar8" else np.uint16


XFORM_TO_SRGB, XFORM_TO_BT709, XFORM_TO_LINEAR = 0, 1, 2
XFORM_TARGETS = {"srgb": XFORM_TO_SRGB, "bt709": XFORM_TO_BT709, "linear": XFORM_TO_LINEAR}


class OutputTransform(C.Structure):
    """vvr_output_transform: the colour transform of the RGB formats, 1-D table -> Q14 3x3 matrix -> 1-D table (vvr_set_output_transform, vvr.h)"""
    _fields_ = [("struct_size", u32), ("pad", u32), ("lin", u16 * 1024), ("m", (i32 * 3) * 3), ("enc", u16 * 1025), ("pad2", u16 * 3)]


def output_transform(lin, m, enc):
    """an OutputTransform from its fields as arrays: lin (1024,) and enc (1025,) uint16, m (3, 3) int32 in Q14"""
    import numpy as np
    t = OutputTransform()
    t.struct_size = C.sizeof(OutputTransform)
    for name, arr, dt in (("lin", lin, np.uint16), ("m", m, np.int32), ("enc", enc, np.uint16)):
        field = getattr(t, name)
        a = np.ascontiguousarray(arr, dtype=dt)
        assert a.nbytes == C.sizeof(field), name
        C.memmove(C.addressof(field), a.ctypes.data, a.nbytes)
    return t


def output_transform_arrays(t):
    """(lin, m, enc) of an OutputTransform as numpy arrays (copies)"""
    import numpy as np
    return np.array(t.lin, np.uint16), np.array([list(r) for r in t.m], np.int32), np.array(t.enc, np.uint16)


LUT3D_SIZES = (17, 33, 65)


def lut3d_nodes(n, nodes):
    """the nodes of a 3-D LUT as vvr_set_output_lut3d takes them: a contiguous uint16 array of n^3 x 3 values in .cube order (R fastest);
    `nodes` may have any shape with that many elements, (n, n, n, 3) indexed [jb, jg, jr] included"""
    import numpy as np
    a = np.ascontiguousarray(nodes, dtype=np.uint16).reshape(-1)
    assert a.size == 3 * int(n) ** 3, "a %d-point LUT has %d values, not %d" % (n, 3 * int(n) ** 3, a.size)
    return a


HASH_MD5, HASH_CRC, HASH_CHECKSUM = 0, 1, 2
HASH_LEN = {HASH_MD5: 16, HASH_CRC: 2, HASH_CHECKSUM: 4}


class HashRequest(C.Structure):
    """vvr_hash_request: a decoded picture hash as a request of the output queue (vvr_hash_submit, vvr.h)"""
    _fields_ = [("struct_size", u32), ("slot", i32), ("job", i32), ("method", u8), ("blocking", u8), ("pad", u8 * 2),
                ("digest", C.c_void_p), ("expected", C.c_void_p), ("mismatch", C.c_void_p)]


STATS_LUMA, STATS_RGB = 0, 1
STATS_MODES = {"luma": STATS_LUMA, "rgb": STATS_RGB}


class FrameStats(C.Structure):
    """vvr_frame_stats: what vvr_output_wait writes for a statistics request (vvr_stats_submit, vvr.h)"""
    _fields_ = [("struct_size", u32), ("mode", u32), ("bit_depth", u32), ("pad", u32), ("width", u32), ("height", u32), ("samples", u64),
                ("hist_y", u32 * 1024), ("hist_maxrgb", u32 * 1024), ("max_c", u32 * 3), ("min_c", u32 * 3)]


class StatsRequest(C.Structure):
    """vvr_stats_request: light-level statistics of a picture as a request of the output queue (vvr_stats_submit, vvr.h)"""
    _fields_ = [("struct_size", u32), ("slot", i32), ("job", i32), ("x", i32), ("y", i32), ("w", i32), ("h", i32),
                ("collocated", u8), ("mode", u8), ("blocking", u8), ("pad", u8), ("stats", C.c_void_p)]


class LightLevel(C.Structure):
    """vvr_light_level: the light levels vvr_light_level derives from RGB-mode statistics (vvr.h)"""
    _fields_ = [("struct_size", u32), ("transfer", u32), ("max_code", u32), ("pct_code", u32),
                ("max_nits", C.c_double), ("pct_nits", C.c_double), ("avg_nits", C.c_double), ("maxscl_nits", C.c_double * 3)]


def stats_request(slot, job, window, mode, collocated, blocking, stats):
    """a StatsRequest that writes into `stats` (a FrameStats the caller keeps alive until the request has been waited for)"""
    r = StatsRequest()
    r.struct_size = C.sizeof(StatsRequest)
    r.slot, r.job = slot, -1 if job is None else job
    r.x, r.y, r.w, r.h = window
    r.collocated = int(bool(collocated[0])) | int(bool(collocated[1])) << 1
    r.mode, r.blocking = STATS_MODES[mode] if isinstance(mode, str) else mode, 1 if blocking else 0
    r.stats = C.addressof(stats)
    return r


class FrameCompare(C.Structure):
    """vvr_frame_compare: what vvr_output_wait writes for a comparison request (vvr_compare_submit, vvr.h)"""
    _fields_ = [("struct_size", u32), ("bit_depth", u32), ("num_components", u32), ("pad", u32), ("width", u32 * 3), ("height", u32 * 3),
                ("samples", u64 * 3), ("differing", u64 * 3), ("sse", u64 * 3), ("sad", u64 * 3),
                ("max_abs", u32 * 3), ("first_x", u32 * 3), ("first_y", u32 * 3), ("pad2", u32)]


class CompareRequest(C.Structure):
    """vvr_compare_request: a picture compared with a reference frame as a request of the output queue (vvr_compare_submit, vvr.h)"""
    _fields_ = [("struct_size", u32), ("slot", i32), ("job", i32), ("x", i32), ("y", i32), ("w", i32), ("h", i32), ("ref_slot", i32),
                ("ref_bytes_per_sample", u8), ("blocking", u8), ("pad", u8 * 2), ("pad2", u32),
                ("ref", C.c_void_p * 3), ("ref_stride_bytes", C.c_size_t * 3), ("result", C.c_void_p), ("map", C.c_void_p)]


def compare_map_shape(window):
    """(rows, columns) of the map of a comparison: one word per block of 64 x 64 luma samples of the window"""
    return (window[3] + 63) // 64, (window[2] + 63) // 64


def compare_request(slot, job, window, ref, result, map_=None, blocking=True, ref_bytes_per_sample=2):
    """a CompareRequest that writes into `result` (a FrameCompare) and, when given, `map_` (a C-contiguous uint32 array of compare_map_shape),
    both kept alive by the caller until the request has been waited for.  ref: a slot number, or per component a numpy plane (uint8 / uint16,
    rows contiguous), an object with data_ptr() / stride() / element_size() (a torch tensor), or an (address, stride in bytes) pair with
    ref_bytes_per_sample"""
    r = CompareRequest()
    r.struct_size = C.sizeof(CompareRequest)
    r.slot, r.job, r.blocking = slot, -1 if job is None else job, 1 if blocking else 0
    r.x, r.y, r.w, r.h = window
    r.ref_slot, r.ref_bytes_per_sample = -1, ref_bytes_per_sample
    if isinstance(ref, int):
        r.ref_slot = ref
    else:
        for k, pl in enumerate(ref):
            if isinstance(pl, tuple):
                r.ref[k], r.ref_stride_bytes[k] = pl
            elif hasattr(pl, "data_ptr"):
                r.ref[k], r.ref_stride_bytes[k], r.ref_bytes_per_sample = pl.data_ptr(), pl.stride(0) * pl.element_size(), pl.element_size()
            else:
                r.ref[k], r.ref_stride_bytes[k], r.ref_bytes_per_sample = pl.ctypes.data, pl.strides[0], pl.itemsize
    r.result = C.addressof(result)
    r.map = None if map_ is None else map_.ctypes.data
    return r


class FrameSsim(C.Structure):
    """vvr_frame_ssim: what vvr_output_wait writes for an SSIM request (vvr_ssim_submit, vvr.h)"""
    _fields_ = [("struct_size", u32), ("bit_depth", u32), ("num_components", u32), ("pad", u32), ("width", u32 * 3), ("height", u32 * 3),
                ("windows_x", u32 * 3), ("windows_y", u32 * 3), ("windows", u64 * 3), ("sum", C.c_int64 * 3), ("min", i32 * 3),
                ("min_x", u32 * 3), ("min_y", u32 * 3), ("pad2", u32)]


class SsimRequest(C.Structure):
    """vvr_ssim_request: SSIM of a picture against a reference frame as a request of the output queue (vvr_ssim_submit, vvr.h); field by field a
    CompareRequest"""
    _fields_ = list(CompareRequest._fields_)


def ssim_map_shape(window):
    """(rows, columns) of the map of an SSIM request: one word per block of 64 x 64 luma samples of the window"""
    return compare_map_shape(window)


def ssim_request(slot, job, window, ref, result, map_=None, blocking=True, ref_bytes_per_sample=2):
    """an SsimRequest that writes into `result` (a FrameSsim) and, when given, `map_` (a C-contiguous int32 array of ssim_map_shape); everything
    else as compare_request"""
    c = compare_request(slot, job, window, ref, result, map_, blocking, ref_bytes_per_sample)
    r = SsimRequest.from_buffer_copy(bytes(c))
    r.struct_size = C.sizeof(SsimRequest)
    return r


MSSSIM_MAX_SCALES = 5
MSSSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)      # Wang et al. 2003; vvr_compare_msssim divides the first `scales` by their sum


class FrameMsssim(C.Structure):
    """vvr_frame_msssim: what vvr_output_wait writes for an MS-SSIM request (vvr_msssim_submit, vvr.h); indices are [level][component]"""
    _fields_ = [("struct_size", u32), ("bit_depth", u32), ("num_components", u32), ("scales", u32),
                ("width", u32 * 3 * 5), ("height", u32 * 3 * 5), ("windows_x", u32 * 3 * 5), ("windows_y", u32 * 3 * 5),
                ("windows", u64 * 3 * 5), ("sum_cs", C.c_int64 * 3 * 5), ("sum_v", C.c_int64 * 3 * 5)]


class MsssimRequest(C.Structure):
    """vvr_msssim_request: MS-SSIM of a picture against a reference frame as a request of the output queue (vvr_msssim_submit, vvr.h): an
    SsimRequest with `scales` where its first pad byte was, and no map"""
    _fields_ = [("struct_size", u32), ("slot", i32), ("job", i32), ("x", i32), ("y", i32), ("w", i32), ("h", i32), ("ref_slot", i32),
                ("ref_bytes_per_sample", u8), ("blocking", u8), ("scales", u8), ("pad", u8), ("pad2", u32),
                ("ref", C.c_void_p * 3), ("ref_stride_bytes", C.c_size_t * 3), ("result", C.c_void_p)]


def msssim_request(slot, job, window, ref, result, scales=5, blocking=True, ref_bytes_per_sample=2):
    """an MsssimRequest of `scales` levels that writes into `result` (a FrameMsssim); everything else as compare_request"""
    c = compare_request(slot, job, window, ref, result, None, blocking, ref_bytes_per_sample)
    r = MsssimRequest.from_buffer_copy(bytes(c)[:C.sizeof(MsssimRequest)])
    r.struct_size, r.scales = C.sizeof(MsssimRequest), scales
    return r


XPSNR_MAX_BLOCKS = 16384


class XpsnrBlock(C.Structure):
    """vvr_xpsnr_block: the record of one block of an XPSNR request (vvr_xpsnr_submit, vvr.h)"""
    _fields_ = [("sse", u64 * 3), ("act_spatial", u64), ("act_temporal", u64), ("count", u32), ("pad", u32)]


XPSNR_BLOCK_FIELDS = [("sse", "<u8", (3,)), ("act_spatial", "<u8"), ("act_temporal", "<u8"), ("count", "<u4"), ("pad", "<u4")]      # an XpsnrBlock as the fields of a numpy dtype


class FrameXpsnr(C.Structure):
    """vvr_frame_xpsnr: what vvr_output_wait writes for an XPSNR request (vvr_xpsnr_submit, vvr.h): the geometry and the sums over the blocks"""
    _fields_ = [("struct_size", u32), ("bit_depth", u32), ("num_components", u32), ("temporal", u32), ("filter", u32), ("block", u32),
                ("blocks_x", u32), ("blocks_y", u32), ("width", u32 * 3), ("height", u32 * 3), ("samples", u64 * 3), ("sse", u64 * 3),
                ("act_spatial", u64), ("act_temporal", u64), ("count", u64)]


class XpsnrRequest(C.Structure):
    """vvr_xpsnr_request: XPSNR of a picture against a reference frame as a request of the output queue (vvr_xpsnr_submit, vvr.h): a
    CompareRequest up to the reference's strides, with temporal and filter in its pad bytes and block in pad2, then the prev planes"""
    _fields_ = [("struct_size", u32), ("slot", i32), ("job", i32), ("x", i32), ("y", i32), ("w", i32), ("h", i32), ("ref_slot", i32),
                ("ref_bytes_per_sample", u8), ("blocking", u8), ("temporal", u8), ("filter", u8), ("block", u32),
                ("ref", C.c_void_p * 3), ("ref_stride_bytes", C.c_size_t * 3), ("prev", C.c_void_p * 2), ("prev_stride_bytes", C.c_size_t * 2),
                ("result", C.c_void_p), ("blocks", C.c_void_p)]


def xpsnr_blocks(w, h, block=0):
    """vvr_xpsnr_blocks restated: (B, blocks_x, blocks_y) of a window of w x h with the request's `block`, or None where the call refuses"""
    if w < 8 or h < 8 or block < 0 or block & 3:
        return None
    b = block or max(4, 4 * int(32.0 * math.sqrt(w * h / 8294400.0) + 0.5))
    bx, by = (w + b - 1) // b, (h + b - 1) // b
    return (b, bx, by) if bx * by <= XPSNR_MAX_BLOCKS else None


def xpsnr_request(slot, job, window, ref, result, prev=(), blocks=None, block=0, filter=0, blocking=True, ref_bytes_per_sample=2):
    """an XpsnrRequest that writes into `result` (a FrameXpsnr) and, when given, `blocks` (a C-contiguous array of np.dtype(XPSNR_BLOCK_FIELDS) with
    blocks_x * blocks_y records); prev: the luma planes o1 (, o2) as compare_request takes the reference's planes, temporal = len(prev);
    everything else as compare_request"""
    c = compare_request(slot, job, window, ref, result, None, blocking, ref_bytes_per_sample)
    r = XpsnrRequest()
    C.memmove(C.addressof(r), C.addressof(c), XpsnrRequest.prev.offset)
    r.struct_size, r.temporal, r.filter, r.block = C.sizeof(XpsnrRequest), len(prev), filter, block
    for k, pl in enumerate(prev):
        if isinstance(pl, tuple):
            r.prev[k], r.prev_stride_bytes[k] = pl
        elif hasattr(pl, "data_ptr"):
            r.prev[k], r.prev_stride_bytes[k] = pl.data_ptr(), pl.stride(0) * pl.element_size()
            if isinstance(ref, int):
                r.ref_bytes_per_sample = pl.element_size()
        else:
            r.prev[k], r.prev_stride_bytes[k] = pl.ctypes.data, pl.strides[0]
            if isinstance(ref, int):
                r.ref_bytes_per_sample = pl.itemsize
    r.result = C.addressof(result)
    r.blocks = None if blocks is None else blocks.ctypes.data
    return r


class KernelStat(C.Structure):
    _fields_ = [("name", C.c_char * 32), ("launches", u64), ("total_ms", C.c_double), ("algo_bytes", C.c_double)]


# The C signatures of include/vvr.h, name -> (restype, argtypes): the one place they are written down.  Pointers to structs, arrays and
# opaque handles are c_void_p (byref(), addresses, arrays and None all pass); the two arrays of vvr_read_output_grain keep their element types.
_int, _p, _sz, _dbl = C.c_int, C.c_void_p, C.c_size_t, C.c_double
_submit = (_int, [_p, _p])
SIGNATURES = {
    "vvr_create": (_int, [_p, _p]),
    "vvr_destroy": (None, [_p]),
    "vvr_submit": _submit,
    "vvr_inputs_done": (_int, [_p, _int]),
    "vvr_host_alloc": (_p, [_p, _sz]),
    "vvr_host_free": (None, [_p, _p]),
    "vvr_wait": (_int, [_p, _int]),
    "vvr_test": (_int, [_p, _int]),
    "vvr_sync": (_int, [_p]),
    "vvr_slot_bytes": (_sz, [_p]),
    "vvr_plane_layout": (_int, [_p, _int, _p, _p, _p, _p]),
    "vvr_plane_ptr": (_p, [_p, _int, _int]),
    "vvr_read_plane": (_int, [_p, _int, _int, _p, _sz]),
    "vvr_read_output": (_int, [_p] + [_int] * 7 + [_p, _sz]),
    "vvr_read_output_scaled": (_int, [_p] + [_int] * 10 + [_p, _sz]),
    "vvr_set_film_grain": _submit,
    "vvr_set_film_grain_seed": (_int, [_p, u32]),
    "vvr_read_output_grain": (_int, [_p] + [_int] * 6 + [C.POINTER(_p), C.POINTER(_sz)]),
    "vvr_set_output_colour": (_int, [_p, _int, _int]),
    "vvr_set_output_narrowing": (_int, [_p, _int, _int]),
    "vvr_set_output_resampling": (_int, [_p, _int]),
    "vvr_resample_taps": (_int, [_int] * 5 + [_p, _p]),
    "vvr_set_output_normalisation": (_int, [_p, _p, _p]),
    "vvr_set_output_transform": _submit,
    "vvr_output_transform_preset": (_int, [_p, _int, _int, _int, _dbl, _dbl, _int]),
    "vvr_set_output_lut3d": (_int, [_p, _int, _p]),
    "vvr_output_lut3d_preset": (_int, [_p, _int, _int, _int, _int, _dbl, _dbl]),
    "vvr_output_submit": _submit,
    "vvr_output_submit_batch": (_int, [_p, _p, _p]),
    "vvr_output_test": (_int, [_p, _int]),
    "vvr_output_wait": (_int, [_p, _int]),
    "vvr_device_alloc": (_p, [_p, _sz]),
    "vvr_device_free": (None, [_p, _p]),
    "vvr_device_register": (_int, [_p, _p, _sz]),
    "vvr_device_unregister": _submit,
    "vvr_output_stream_wait": (_int, [_p, _int, _p]),
    "vvr_picture_hash": (_int, [_p, _int, _int, _p, _p]),
    "vvr_hash_submit": _submit,
    "vvr_stats_submit": _submit,
    "vvr_light_level": (_int, [_p, _int, u32, _p]),
    "vvr_compare_submit": _submit,
    "vvr_compare_psnr": (_int, [_p, _dbl, _p]),
    "vvr_ssim_submit": _submit,
    "vvr_compare_ssim": (_int, [_p, _p]),
    "vvr_msssim_submit": _submit,
    "vvr_compare_msssim": (_int, [_p, _p, _p]),
    "vvr_xpsnr_submit": _submit,
    "vvr_xpsnr_blocks": (_int, [_int, _int, u32, _p, _p, _p]),
    "vvr_compare_xpsnr": (_int, [_p, _p, _dbl, _dbl, _p]),
    "vvr_set_compare_scaling": (_int, [_p, _int, _int, _int]),
    "vvr_read_picture": (_int, [_p, _int, _p, _p, _int]),
    "vvr_write_plane": (_int, [_p, _int, _int, _p, _sz]),
    "vvr_slot_picture_size": (_int, [_p, _int, _int, _int]),
    "vvr_read_dmvr": (_int, [_p, _int, _p, _sz]),
    "vvr_read_col_motion": (_int, [_p, _int, _p, _sz]),
    "vvr_prepare": (_int, [_p, _p, _p]),
    "vvr_submit_prepared": _submit,
    "vvr_free_prepared": (None, [_p, _p]),
    "vvr_job_stream": (_p, [_p, _int]),
    "vvr_stream_wait_job": (_int, [_p, _int, _p, _int]),
    "vvr_stream_wait_slot": (_int, [_p, _int, _p, _int]),
    "vvr_slot_external_event": (_int, [_p, _int, _p, _int]),
    "vvr_last_error": (C.c_char_p, [_p]),
    "vvr_version": (C.c_char_p, []),
    "vvr_abi_sizeof": (_sz, [_int]),
    "vvr_enable_stats": (_int, [_p, _int]),
    "vvr_get_stats": (_int, [_p, _p, _int]),
    "vvr_measure_copy_bandwidth": (_dbl, [_p, _int]),
    "vvr_resolve_tr_type": (u8, [_p, _p, _p, _int, _int, _int, _int]),
}


def bind(L):
    """the signatures of SIGNATURES on a loaded library (the product's, or the host build of the tests, which exports the same vvr_* names); a
    missing symbol is an AttributeError"""
    return _bind_names(L, *SIGNATURES)


def _bind_names(L, *names):
    for name in names:
        f = getattr(L, name)
        f.restype, f.argtypes = SIGNATURES[name][0], list(SIGNATURES[name][1])
    return L


# the per-feature helpers of earlier callers: the same table, a few names at a time
def bind_output_narrowing(L):
    return _bind_names(L, "vvr_set_output_narrowing")


def bind_output_resampling(L):
    return _bind_names(L, "vvr_set_output_resampling", "vvr_resample_taps")


def bind_compare_scaling(L):
    return _bind_names(L, "vvr_set_compare_scaling")


def bind_output_batch(L):
    return _bind_names(L, "vvr_output_submit_batch")

