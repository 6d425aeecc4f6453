"""TEST INFRASTRUCTURE: the reference's own vvdec::rescalePlane (vvdecimpl.cpp:1620, the one C++ function the drop-in library oracle/_ref/libvvdec.so
exports besides its C API) on a batch of planes, in a child process: rescalePlane calls g_pelBufOP.sampleRateConv, which is the plain C++
sampleRateConvCore (Buffer.cpp:235) until a decoder is opened and the x86 SIMD version (BufferX86.h:1799) after that, for the rest of the process.
So each path gets a fresh process.  The drop-in's vvr_* references resolve to the back-end loaded before it (RTLD_GLOBAL): the product library on
a GPU machine, the stand-in build of tests/hoststub on the CPU.

    python tests/rescale_ref.py <back-end library> <simd 0|1> <cases.npz> <out.npz>

    python tests/rescale_ref.py --decode <back-end library> <stream.bit> <frames.npz>

decodes a bitstream in-process through the drop-in's vvdec_* C API and saves every output frame (cropped planes as uint16, sizes, the sequence's
maximum size and the chroma sample position vvdecapp's upscaleFrame derives from the VUI, vvdecHelper.h:978-1010).

cases.npz: for case n, src<n> (uint16, h x w) and par<n> = [out_w, out_h, comp, color_format, bit_depth, hor_collocated, ver_collocated];
out.npz: out<n> (uint16, out_h x out_w)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
DROPIN_LIB = os.path.join(HERE, "..", "oracle", "_ref", "libvvdec.so")
RESCALE = "_ZN5vvdec12rescalePlaneERK10vvdecPlaneRS0_i16vvdecColorFormatibb"


def available():
    return os.path.exists(DROPIN_LIB)


class Plane(C.Structure):          # vvdecPlane (vvdec.h.in:454-462)
    _fields_ = [("ptr", C.c_void_p), ("width", C.c_uint32), ("height", C.c_uint32), ("stride", C.c_uint32), ("bytesPerSample", C.c_uint32), ("allocator", C.c_void_p)]


class Params(C.Structure):         # vvdecParams (vvdec.h.in:487-502)
    _fields_ = [("threads", C.c_int), ("parseDelay", C.c_int), ("logLevel", C.c_int), ("verifyPictureHash", C.c_bool), ("filmGrainSynthesis", C.c_bool),
                ("simd", C.c_int), ("opaque", C.c_void_p), ("errHandlingFlags", C.c_int), ("reserved", C.c_int32 * 4)]


# (source, output) sides per axis: ratios 2, 1.5, 4/3, 1, 1/2, 1/8, 8, odd ones, sources of 1 and 2 samples
AXES = [(32, 64), (32, 48), (24, 32), (40, 40), (64, 32), (64, 8), (8, 64), (383, 1001), (1, 8), (2, 16), (2, 1), (17, 9)]


def matrix(chroma_format):
    """windows of the case matrix: (comp, x, y, w, h, out_w, out_h, collocated bits) in samples of the component; windows at odd and even
    offsets, every axis pair of AXES once horizontally and once vertically, the equal-size copy, all four chroma sample positions"""
    pairs = [(AXES[k], AXES[(k + 3) % len(AXES)]) for k in range(len(AXES))] + [((40, 40), (40, 40))]
    out = []
    for k, ((w, ow), (h, oh)) in enumerate(pairs):
        x, y = 2 * k + 1, k + 2
        out.append((0, x, y, w, h, ow, oh, k & 3))             # (luma: always collocated, the bits are ignored)
        if chroma_format:
            for col in range(4):
                out.append((1 + (col & 1), x + col, y, w, h, ow, oh, col))
    return out


class Vui(C.Structure):            # vvdecVui (vvdec.h.in:345-369)
    _fields_ = [("aspectRatioInfoPresentFlag", C.c_bool), ("aspectRatioConstantFlag", C.c_bool), ("nonPackedFlag", C.c_bool), ("nonProjectedFlag", C.c_bool),
                ("aspectRatioIdc", C.c_int), ("sarWidth", C.c_int), ("sarHeight", C.c_int), ("colourDescriptionPresentFlag", C.c_bool), ("colourPrimaries", C.c_int),
                ("transferCharacteristics", C.c_int), ("matrixCoefficients", C.c_int), ("progressiveSourceFlag", C.c_bool), ("interlacedSourceFlag", C.c_bool),
                ("chromaLocInfoPresentFlag", C.c_bool), ("chromaSampleLocTypeTopField", C.c_int), ("chromaSampleLocTypeBottomField", C.c_int),
                ("chromaSampleLocType", C.c_int), ("overscanInfoPresentFlag", C.c_bool), ("overscanAppropriateFlag", C.c_bool),
                ("videoSignalTypePresentFlag", C.c_bool), ("videoFullRangeFlag", C.c_bool)]


class SeqInfo(C.Structure):        # vvdecSeqInfo (vvdec.h.in:415-426)
    _fields_ = [("maxWidth", C.c_uint32), ("maxHeight", C.c_uint32)]


class PicAttributes(C.Structure):  # vvdecPicAttributes (vvdec.h.in:431-447), up to seqInfo
    _fields_ = [("nalType", C.c_int), ("sliceType", C.c_int), ("isRefPic", C.c_bool), ("temporalLayer", C.c_uint32), ("poc", C.c_int64), ("bits", C.c_uint32),
                ("vui", C.POINTER(Vui)), ("hrd", C.c_void_p), ("olsHrd", C.c_void_p), ("seqInfo", C.POINTER(SeqInfo))]


class Frame(C.Structure):          # vvdecFrame (vvdec.h.in:468-481)
    _fields_ = [("planes", Plane * 3), ("numPlanes", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("bitDepth", C.c_uint32), ("frameFormat", C.c_int),
                ("colorFormat", C.c_int), ("sequenceNumber", C.c_uint64), ("cts", C.c_uint64), ("ctsValid", C.c_bool), ("picAttributes", C.POINTER(PicAttributes))]


class AccessUnit(C.Structure):     # vvdecAccessUnit (vvdec.h.in:300-313)
    _fields_ = [("payload", C.POINTER(C.c_ubyte)), ("payloadSize", C.c_int), ("payloadUsedSize", C.c_int), ("cts", C.c_uint64), ("dts", C.c_uint64),
                ("ctsValid", C.c_bool), ("dtsValid", C.c_bool), ("rap", C.c_bool)]


def chroma_collocation(fr):
    """upscaleFrame (vvdecHelper.h:978-1010): 4:2:0 default horizontal collocated, vertical not; BT.2020 primaries (9): vertical collocated;
    chromaSampleLocType 0..3 when the VUI carries it (6: unspecified, the default stays); other formats: both collocated"""
    hor, ver = True, True
    if fr.colorFormat == 1:
        hor, ver = True, False
        vui = fr.picAttributes.contents.vui if fr.picAttributes else None
        if vui and vui.contents.colourPrimaries == 9:
            ver = True
        if vui and vui.contents.chromaLocInfoPresentFlag:
            t = vui.contents.chromaSampleLocType
            assert t in (0, 1, 2, 3, 6), "chromaSampleLocType %d: vvdecapp does not rescale" % t
            if t != 6:
                hor, ver = t in (0, 2), t in (2, 3)
    return hor, ver


def _decode(backend, bit, cout):
    C.CDLL(backend, mode=C.RTLD_GLOBAL)
    L = C.CDLL(DROPIN_LIB)
    L.vvdec_params_alloc.restype = C.POINTER(Params)
    L.vvdec_decoder_open.restype = C.c_void_p
    L.vvdec_decoder_open.argtypes = [C.POINTER(Params)]
    L.vvdec_decoder_close.argtypes = [C.c_void_p]
    L.vvdec_accessUnit_alloc.restype = C.POINTER(AccessUnit)
    L.vvdec_accessUnit_alloc_payload.argtypes = [C.POINTER(AccessUnit), C.c_int]
    L.vvdec_accessUnit_free.argtypes = [C.POINTER(AccessUnit)]
    L.vvdec_decode.argtypes = [C.c_void_p, C.POINTER(AccessUnit), C.POINTER(C.POINTER(Frame))]
    L.vvdec_flush.argtypes = [C.c_void_p, C.POINTER(C.POINTER(Frame))]
    L.vvdec_frame_unref.argtypes = [C.c_void_p, C.POINTER(Frame)]
    p = L.vvdec_params_alloc()
    L.vvdec_params_default(p)
    p.contents.threads = 2
    p.contents.logLevel = 0
    dec = L.vvdec_decoder_open(p)
    assert dec, "vvdec_decoder_open failed"
    data = open(bit, "rb").read()
    # NAL units with their start codes, one per call (readBitstreamFromFile of vvdecapp hands them over the same way)
    starts, i = [], data.find(b"\x00\x00\x01")
    while i >= 0:
        starts.append(i - 1 if i > 0 and data[i - 1] == 0 else i)
        i = data.find(b"\x00\x00\x01", i + 3)
    nals = [data[a:b] for a, b in zip(starts, starts[1:] + [len(data)])]
    au = L.vvdec_accessUnit_alloc()
    L.vvdec_accessUnit_alloc_payload(au, max(len(n) for n in nals) + 16)
    out, n = {}, 0

    def take(fr):
        nonlocal n
        f = fr.contents
        for c in range(f.numPlanes):
            pl = f.planes[c]
            raw = np.frombuffer(C.string_at(pl.ptr, pl.stride * pl.height), np.uint8 if pl.bytesPerSample == 1 else np.uint16)
            out["f%d_c%d" % (n, c)] = raw.reshape(pl.height, pl.stride // pl.bytesPerSample)[:, :pl.width].astype(np.uint16)
        seq = f.picAttributes.contents.seqInfo if f.picAttributes else None
        hor, ver = chroma_collocation(f)
        out["f%d_par" % n] = np.array([f.numPlanes, f.width, f.height, f.bitDepth, f.frameFormat, f.colorFormat, seq.contents.maxWidth if seq else 0,
                                       seq.contents.maxHeight if seq else 0, int(hor), int(ver)], np.int64)
        n += 1
        L.vvdec_frame_unref(dec, fr)
    for nal in nals:
        C.memmove(au.contents.payload, nal, len(nal))
        au.contents.payloadUsedSize = len(nal)
        fr = C.POINTER(Frame)()
        rc = L.vvdec_decode(dec, au, C.byref(fr))
        assert rc in (0, -40), "vvdec_decode: %d" % rc
        if fr:
            take(fr)
    while True:
        fr = C.POINTER(Frame)()
        rc = L.vvdec_flush(dec, C.byref(fr))
        if fr:
            take(fr)
        if rc == -50 or not fr:
            break
        assert rc == 0, "vvdec_flush: %d" % rc
    L.vvdec_accessUnit_free(au)
    assert L.vvdec_decoder_close(dec) == 0
    np.savez(cout, **out)


def decode(backend, bit, tmpdir):
    """-> list of frames: dict(planes, width, height, bit_depth, progressive, color_format, max_width, max_height, collocated) in output order"""
    cout = os.path.join(tmpdir, os.path.basename(bit) + ".frames.npz")
    subprocess.check_call([sys.executable, os.path.abspath(__file__), "--decode", backend, bit, cout], timeout=1200)
    got = np.load(cout)
    frames, n = [], 0
    while "f%d_par" % n in got:
        np_, w, h, bd, ff, cf, mw, mh, hor, ver = (int(v) for v in got["f%d_par" % n])
        frames.append(dict(planes=[got["f%d_c%d" % (n, c)] for c in range(np_)], width=w, height=h, bit_depth=bd, progressive=ff == 0, color_format=cf,
                           max_width=mw, max_height=mh, collocated=(bool(hor), bool(ver))))
        n += 1
    return frames


def rescale(cases, backend, simd, tmpdir):
    """cases: list of (src uint16 h x w, out_w, out_h, comp, color_format, bit_depth, hor, ver) -> list of uint16 arrays, by rescalePlane on the
    plain C++ path (simd False) or the SIMD path (simd True)"""
    cin, cout = os.path.join(tmpdir, "rescale_cases.npz"), os.path.join(tmpdir, "rescale_out_%d.npz" % int(simd))
    arrs = {}
    for n, (src, ow, oh, comp, cf, bd, hor, ver) in enumerate(cases):
        arrs["src%d" % n] = np.ascontiguousarray(src, dtype=np.uint16)
        arrs["par%d" % n] = np.array([ow, oh, comp, cf, bd, int(hor), int(ver)], np.int64)
    np.savez(cin, **arrs)
    subprocess.check_call([sys.executable, os.path.abspath(__file__), backend, str(int(simd)), cin, cout], timeout=1200)
    got = np.load(cout)
    return [got["out%d" % n] for n in range(len(cases))]


def _main(backend, simd, cin, cout):
    C.CDLL(backend, mode=C.RTLD_GLOBAL)
    L = C.CDLL(DROPIN_LIB)
    f = getattr(L, RESCALE)
    f.restype = None
    f.argtypes = [C.POINTER(Plane), C.POINTER(Plane), C.c_int, C.c_int, C.c_int, C.c_bool, C.c_bool]
    dec = None
    if simd:
        # opening a decoder installs the SIMD buffer operations (DecLibRecon constructor, the drop-in's as the reference's)
        L.vvdec_params_alloc.restype = C.POINTER(Params)
        L.vvdec_decoder_open.restype = C.c_void_p
        L.vvdec_decoder_open.argtypes = [C.POINTER(Params)]
        L.vvdec_decoder_close.argtypes = [C.c_void_p]
        p = L.vvdec_params_alloc()
        L.vvdec_params_default(p)
        p.contents.threads = 0
        p.contents.logLevel = 0
        dec = L.vvdec_decoder_open(p)
        assert dec, "vvdec_decoder_open failed"
    cases = np.load(cin)
    out = {}
    n = 0
    while "src%d" % n in cases:
        src = np.ascontiguousarray(cases["src%d" % n])
        ow, oh, comp, cf, bd, hor, ver = (int(v) for v in cases["par%d" % n])
        dst = np.zeros((oh, ow), np.uint16)
        sp = Plane(src.ctypes.data, src.shape[1], src.shape[0], src.strides[0], 2, None)
        dp = Plane(dst.ctypes.data, ow, oh, dst.strides[0], 2, None)
        f(C.byref(sp), C.byref(dp), comp, cf, bd, bool(hor), bool(ver))
        out["out%d" % n] = dst
        n += 1
    np.savez(cout, **out)
    if dec:
        L.vvdec_decoder_close(dec)


if __name__ == "__main__":
    if sys.argv[1] == "--decode":
        _decode(sys.argv[2], sys.argv[3], sys.argv[4])
        sys.exit(0)
    _main(sys.argv[1], int(sys.argv[2]), sys.argv[3], sys.argv[4])
