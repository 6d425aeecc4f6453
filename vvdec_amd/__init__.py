"""vvdec_amd — MI355X-native VVC (H.266) reconstruction back-end.

Python is only plumbing here (ctypes binding of the C ABI in include/vvr.h, used by tests, bench.py and the multi-GPU
launcher).  The product is `libvvdec_amd.so`: hand-written HIP kernels for gfx950 + the C++ host scheduler in
vvdec_amd/csrc/.  There is no CPU fallback: if the library is missing or no gfx950 device is present, creating a
`Reconstructor` raises.

`Reconstructor` mirrors the reference's DecLibRecon (source/Lib/DecoderLib/DecLibRecon.h:143-200):
    create / destroy               -> Reconstructor(...) / close()
    decompressPicture(Picture*)    -> decompress_picture(desc)        (asynchronous, returns a job id)
    waitForPrevDecompressedPic()   -> wait(job)
"""
import ctypes as C
import os
import subprocess
import numpy as np
from . import abi
from .desc import PictureDesc

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIBPATH = os.environ.get("VVDEC_AMD_LIB") or os.path.join(_HERE, "libvvdec_amd.so")      # (VVDEC_AMD_LIB: developer builds of the same library, e.g. `make watchdog`)
_lib = None


class VvrError(RuntimeError):
    pass


def build(force=False):
    """Compile the HIP library for gfx950 (hipcc cross-compiles without a GPU)."""
    src = os.path.join(_HERE, "csrc")
    if force and os.path.exists(_LIBPATH):
        os.remove(_LIBPATH)
    subprocess.check_call(["make", "-C", src], stdout=subprocess.DEVNULL)
    return _LIBPATH


def lib():
    """The loaded C-ABI library; raises if it has not been built (never falls back to a CPU path)."""
    global _lib
    if _lib is None:
        if not os.path.exists(_LIBPATH):
            raise VvrError("libvvdec_amd.so is missing: run `python -c 'import __graft_entry__ as g; g.build()'` (no CPU fallback exists)")
        _lib = abi.bind(C.CDLL(_LIBPATH))
    return _lib


EXPORTED_SYMBOLS = ["vvr_version", "vvr_create", "vvr_destroy", "vvr_submit", "vvr_wait", "vvr_test", "vvr_sync", "vvr_slot_bytes", "vvr_plane_layout",
                    "vvr_plane_ptr", "vvr_read_plane", "vvr_read_output", "vvr_read_output_scaled", "vvr_set_film_grain", "vvr_set_film_grain_seed", "vvr_set_output_colour", "vvr_set_output_narrowing", "vvr_set_output_resampling", "vvr_resample_taps", "vvr_set_compare_scaling", "vvr_set_output_normalisation", "vvr_set_output_transform", "vvr_output_transform_preset", "vvr_set_output_lut3d", "vvr_output_lut3d_preset", "vvr_read_output_grain", "vvr_picture_hash", "vvr_write_plane", "vvr_read_dmvr", "vvr_read_col_motion", "vvr_prepare", "vvr_submit_prepared",
                    "vvr_free_prepared", "vvr_job_stream", "vvr_last_error", "vvr_enable_stats", "vvr_get_stats", "vvr_resolve_tr_type", "vvr_abi_sizeof",
                    "vvr_inputs_done", "vvr_measure_copy_bandwidth", "vvr_host_alloc", "vvr_host_free",
                    "vvr_stream_wait_job", "vvr_stream_wait_slot", "vvr_slot_external_event", "vvr_slot_picture_size", "vvr_read_picture",
                    "vvr_output_submit", "vvr_output_submit_batch", "vvr_output_test", "vvr_output_wait", "vvr_output_stream_wait", "vvr_hash_submit", "vvr_stats_submit", "vvr_light_level",
                    "vvr_compare_submit", "vvr_compare_psnr", "vvr_ssim_submit", "vvr_compare_ssim", "vvr_msssim_submit", "vvr_compare_msssim",
                    "vvr_xpsnr_submit", "vvr_xpsnr_blocks", "vvr_compare_xpsnr",
                    "vvr_device_alloc", "vvr_device_free", "vvr_device_register", "vvr_device_unregister"]


def resample_taps(filter, n, m, phase, i):
    """vvr_resample_taps: the taps of output sample i of one axis under a filter of Reconstructor.set_output_resampling ("area", "triangle",
    "cubic" or 1 .. 3), n source and m output samples; phase 2 for luma and for chroma that is not collocated on the axis, 1 for chroma that is
    -> (first, [weights]): source samples first .. first + len( weights ) - 1, weights that sum to 16384.  A pure host function: no context, no
    device.  Raises ValueError for what the call refuses (filter 0, sizes outside 1/64 .. 8, i outside 0 .. m - 1)."""
    got = abi.resample_taps(lib(), filter, n, m, phase, i)
    if got is None:
        raise ValueError("resample_taps: refused (filter %r, %r -> %r samples, phase %r, sample %r)" % (filter, n, m, phase, i))
    return got


def output_transform(transfer, primaries, target, src_peak=1000., dst_peak=100., bit_depth=10):
    """vvr_output_transform_preset: the tables that bring HDR video to BT.709 primaries -> an abi.OutputTransform for
    Reconstructor.set_output_transform.  transfer: H.273 transfer_characteristics 16 (PQ) or 18 (HLG); primaries: colour_primaries 9 (BT.2020)
    or 1 (BT.709); target: "srgb", "bt709" (the BT.709 OETF) or "linear" (or abi.XFORM_TO_*); src_peak, dst_peak: cd/m2, the peaks the
    BT.2390 EETF maps between (PQ only); bit_depth: the context's, 8 .. 10.  A pure host function: no context, no device."""
    t = abi.OutputTransform()
    rc = lib().vvr_output_transform_preset(C.byref(t), int(transfer), int(primaries), abi.XFORM_TARGETS.get(target, target), float(src_peak), float(dst_peak), int(bit_depth))
    if rc != abi.VVR_OK:
        raise VvrError("vvr_output_transform_preset: transfer 16 or 18, primaries 1 or 9, a target of abi.XFORM_TARGETS, peaks in (0, 10000], bit depth 8 .. 10 (rc %d)" % rc)
    return t


def output_lut3d(n, transfer, primaries, target, src_peak=1000., dst_peak=100.):
    """vvr_output_lut3d_preset: the 3-D LUT that brings HDR video to BT.709 primaries with the tone curve on luminance (the BT.2390 EETF on Y for
    PQ, the HLG OOTF with the system gamma of a dst_peak display) -> (n, uint16 nodes of n^3 x 3 values in .cube order) for
    Reconstructor.set_output_lut3d, used without a transform.  n: 17, 33 or 65; the other arguments as output_transform's.  A pure host function."""
    import numpy as np
    nodes = np.zeros(3 * int(n) ** 3 if n in abi.LUT3D_SIZES else 3, np.uint16)
    rc = lib().vvr_output_lut3d_preset(nodes.ctypes.data, int(n), int(transfer), int(primaries), abi.XFORM_TARGETS.get(target, target), float(src_peak), float(dst_peak))
    if rc != abi.VVR_OK:
        raise VvrError("vvr_output_lut3d_preset: n 17, 33 or 65, transfer 16 or 18, primaries 1 or 9, a target of abi.XFORM_TARGETS, peaks in (0, 10000] (rc %d)" % rc)
    return int(n), nodes


class FrameStats:
    """the result of Reconstructor.stats_wait: numpy views of the arrays of an abi.FrameStats (`raw`, which light_level takes) and its header
    fields"""
    def __init__(self, raw):
        import numpy as np
        self.raw = raw
        self.mode, self.bit_depth, self.width, self.height, self.samples = raw.mode, raw.bit_depth, raw.width, raw.height, raw.samples
        self.hist_y, self.hist_maxrgb = np.ctypeslib.as_array(raw.hist_y), np.ctypeslib.as_array(raw.hist_maxrgb)
        self.max_c, self.min_c = np.ctypeslib.as_array(raw.max_c), np.ctypeslib.as_array(raw.min_c)


def light_level(stats, transfer=16, percentile=9995):
    """vvr_light_level: the light levels of a frame from its RGB-mode statistics (a FrameStats of stats_wait, or an abi.FrameStats) -> an
    abi.LightLevel: max_code and pct_code (the highest non-empty bin of max( R, G, B ) and its percentile; `percentile` is in units of 0.01 %,
    1 .. 10000, 9995 meaning 99.95 %), and for transfer 16 (PQ) max_nits, pct_nits, avg_nits (the frame average of maxRGB: what MaxFALL is the
    maximum of) and maxscl_nits per channel in cd/m2; transfer 0: the codes alone.  pct_nits is what output_lut3d takes as src_peak for this
    frame.  A pure host function; nothing is computed here."""
    out = abi.LightLevel()
    rc = lib().vvr_light_level(C.byref(getattr(stats, "raw", stats)), int(transfer), int(percentile), C.byref(out))
    if rc != abi.VVR_OK:
        raise VvrError("vvr_light_level: RGB-mode statistics, transfer 16 (PQ) or 0 (codes only), a percentile of 1 .. 10000 (rc %d)" % rc)
    return out


def _cube_tokens(path):
    with open(path) as f:
        for line in f:
            line = line.split("#", 1)[0].strip()
            if line:
                yield line.split()


def read_cube(path):
    """a .cube 3-D LUT file -> (n, uint16 nodes) for Reconstructor.set_output_lut3d: LUT_3D_SIZE 17, 33 or 65 with the default domain (0 .. 1;
    a DOMAIN_MIN / DOMAIN_MAX line must say just that), n^3 rows of R G B with R changing fastest; TITLE and comments are skipped.  Values are
    clipped to [0, 1] and quantised as q16( v ) = floor( v * 65535 + 0.5 ).  Nodes are taken as they are: the file's node j belongs to the input
    j / ( n - 1 ), ours to j * S / 65535 with S = 65536 / ( n - 1 ) - the two grids differ by j / ( ( n - 1 ) * 65535 ), a domain error below
    2^-16 of the range, which is not resampled away."""
    import numpy as np
    n, rows = None, []
    for tok in _cube_tokens(path):
        key = tok[0].upper()
        if key == "LUT_3D_SIZE":
            n = int(tok[1])
        elif key in ("DOMAIN_MIN", "DOMAIN_MAX"):
            if [float(v) for v in tok[1:4]] != [0. if key == "DOMAIN_MIN" else 1.] * 3:
                raise ValueError("read_cube: %s: only the default domain 0 .. 1 is supported" % path)
        elif key == "LUT_1D_SIZE" or key.startswith("LUT_1D") or key.startswith("LUT_3D_INPUT_RANGE"):
            raise ValueError("read_cube: %s: %s is not supported" % (path, tok[0]))
        elif key == "TITLE":
            continue
        else:
            rows.append([float(v) for v in tok[:3]])
            if len(tok) != 3:
                raise ValueError("read_cube: %s: a row of %d values" % (path, len(tok)))
    if n not in abi.LUT3D_SIZES:
        raise ValueError("read_cube: %s: LUT_3D_SIZE %r, not 17, 33 or 65" % (path, n))
    if len(rows) != n ** 3:
        raise ValueError("read_cube: %s: %d rows for a %d-point LUT" % (path, len(rows), n))
    v = np.clip(np.array(rows, np.float64), 0, 1)
    return n, np.floor(v * 65535 + 0.5).astype(np.uint16).reshape(-1)


def write_cube(path, n, nodes, title=None):
    """(n, uint16 nodes) -> a .cube file with the default domain: node values as v / 65535 with 10 decimals, which read_cube brings back exactly"""
    a = abi.lut3d_nodes(n, nodes).reshape(-1, 3)
    with open(path, "w") as f:
        if title:
            f.write('TITLE "%s"\n' % title)
        f.write("LUT_3D_SIZE %d\n" % n)
        for r, g, b in a.tolist():
            f.write("%.10f %.10f %.10f\n" % (r / 65535, g / 65535, b / 65535))


class Reconstructor:
    def __init__(self, width, height, bit_depth=10, log2_ctu=7, chroma_format=1, num_slots=8, num_streams=2, device=0, ext_planes=None, host_threads=0, stop_after=0, ring_entries=0):
        self.L = lib()
        cfg = abi.Config()
        cfg.abi_version = abi.VVR_ABI_VERSION
        cfg.device, cfg.max_width, cfg.max_height = device, width, height
        cfg.chroma_format, cfg.bit_depth, cfg.log2_ctu = chroma_format, bit_depth, log2_ctu
        cfg.num_slots, cfg.num_streams, cfg.host_threads, cfg.stop_after, cfg.ring_entries = num_slots, num_streams, host_threads, stop_after, ring_entries
        cfg.ext_planes = ext_planes
        self.cfg = cfg
        self.ctx = C.c_void_p()
        rc = self.L.vvr_create(C.byref(cfg), C.byref(self.ctx))
        if rc != abi.VVR_OK:
            raise VvrError("vvr_create failed with %d (%s)" % (rc, {abi.VVR_ERR_NO_DEVICE: "no gfx950 device; there is no CPU fallback"}.get(rc, "see include/vvr.h")))
        self.width, self.height, self.chroma_format = width, height, chroma_format
        self._keep = {}
        self._out = {}
        self._reg = {}      # ticket -> addresses registered for the life of the request (output_submit(into=...))
        self._dev = []      # (address, bytes) of device_array memory: known to the context already
        self._compare_scaling = None      # (w, h) of set_compare_scaling, None: off

    # -- lifetime
    def close(self):
        if self.ctx:
            self.L.vvr_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc < 0:
            raise VvrError("vvr error %d: %s" % (rc, self.L.vvr_last_error(self.ctx).decode()))
        return rc

    # -- DecLibRecon interface
    def decompress_picture(self, d: PictureDesc):
        p = d.c()
        job = self._check(self.L.vvr_submit(self.ctx, C.byref(p)))
        self._keep[job] = (d, p)
        return job

    def submit_c(self, p):
        """vvr_submit of a ctypes abi.Picture built beforehand (`desc.c()`); the caller keeps the description alive until wait()"""
        return self._check(self.L.vvr_submit(self.ctx, C.byref(p)))

    def test(self, job):
        """vvr_test: True when `job` is reconstructed (wait() returns at once), False when it is not yet; raises if it failed"""
        rc = self.L.vvr_test(self.ctx, job)
        if rc == abi.VVR_NOT_READY:
            return False
        self._check(rc)
        return True

    def wait(self, job):
        try:
            self._check(self.L.vvr_wait(self.ctx, job))
        finally:
            self._keep.pop(job, None)

    # -- external users of DPB slots, ordered on the device (the collective of vvdec_amd.parallel.PictureParallel)
    def stream_wait_job(self, job, stream_ptr, blocking=True):
        """the caller's stream waits for picture `job`; False: not handed to the device yet (blocking=False only)"""
        return self._check(self.L.vvr_stream_wait_job(self.ctx, job, stream_ptr, 1 if blocking else 0)) == abi.VVR_OK

    def stream_wait_slot(self, slot, stream_ptr, blocking=True):
        """the caller's stream waits for every picture submitted so far that reads or writes `slot`; False: some of them are still being prepared"""
        return self._check(self.L.vvr_stream_wait_slot(self.ctx, slot, stream_ptr, 1 if blocking else 0)) == abi.VVR_OK

    def slot_external_event(self, slot, event_ptr, writes):
        """pictures submitted from now on that use `slot` wait for the caller's event first"""
        self._check(self.L.vvr_slot_external_event(self.ctx, slot, event_ptr, 1 if writes else 0))

    def inputs_done(self, job):
        self._check(self.L.vvr_inputs_done(self.ctx, job))

    def host_array(self, n, dtype):
        """numpy array of n records in host memory the device reads directly (vvr_host_alloc): descriptions built in such arrays are
        uploaded without a staging copy.  The memory belongs to the context (freed by close())."""
        dt = np.dtype(dtype)
        nbytes = max(1, int(n)) * dt.itemsize
        ptr = self.L.vvr_host_alloc(self.ctx, nbytes)
        if not ptr:
            raise VvrError("vvr_host_alloc(%d) failed" % nbytes)
        return np.frombuffer((C.c_char * nbytes).from_address(ptr), dt, count=max(1, int(n)))[:int(n)]

    def device_array(self, nbytes):
        """uint8 torch tensor of nbytes in device memory of the context (vvr_device_alloc): a destination for output_submit(into=...) that
        needs no registration.  The memory belongs to the context: the tensor is a view valid until close().  A process that uses torch tensors
        with a context imports torch before it creates the first context (torch brings its own HIP runtime, which has to be the first one the
        process initialises - the order bench.py uses); otherwise torch finds no device."""
        import torch
        nbytes = max(1, int(nbytes))
        ptr = self.L.vvr_device_alloc(self.ctx, nbytes)
        if not ptr:
            raise VvrError("vvr_device_alloc(%d) failed" % nbytes)
        self._dev.append((ptr, nbytes))

        class _Mem:
            __cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 2, "strides": None}
        return torch.as_tensor(_Mem(), device="cuda:%d" % self.cfg.device)

    def copy_bandwidth(self, iters=20):
        """practical HBM ceiling: bytes/s (read + written) of the library's copy kernel over one DPB slot"""
        return self.L.vvr_measure_copy_bandwidth(self.ctx, iters)

    def sync(self):
        self._check(self.L.vvr_sync(self.ctx))
        self._keep.clear()

    def read_dmvr(self, job, n):
        """delta MVs (n x 2 int32, 1/16 sample) DMVR produced for job's picture, indexed cu.dmvr_off + sub-block"""
        a = np.zeros((max(1, n), 2), np.int32)
        self._check(self.L.vvr_read_dmvr(self.ctx, job, a.ctypes.data, n))
        return a[:n]

    def read_col_motion(self, job):
        """collocated motion of a picture submitted with TOOL_COL_MOTION: abi.Motion records, ((h4 + 1) // 2) * ((w4 + 1) // 2) of them in raster order"""
        n = self._check(self.L.vvr_read_col_motion(self.ctx, job, None, 0))
        a = np.zeros(n, np.dtype(abi.Motion))
        if n:
            self._check(self.L.vvr_read_col_motion(self.ctx, job, a.ctypes.data, n))
        return a

    # -- resident pictures (pre-parsed stream already in HBM)
    def prepare(self, d: PictureDesc):
        p = d.c()
        h = C.c_void_p()
        self._check(self.L.vvr_prepare(self.ctx, C.byref(p), C.byref(h)))
        return h

    def submit_prepared(self, handle):
        return self._check(self.L.vvr_submit_prepared(self.ctx, handle))

    def free_prepared(self, handle):
        self.L.vvr_free_prepared(self.ctx, handle)

    # -- planes
    def plane_shape(self, comp):
        return (self.height >> (1 if comp else 0), self.width >> (1 if comp else 0))

    def read_picture(self, slot):
        out = []
        for c in range(3 if self.chroma_format else 1):
            a = np.zeros(self.plane_shape(c), np.uint16)
            self._check(self.L.vvr_read_plane(self.ctx, slot, c, a.ctypes.data, a.shape[1]))
            out.append(a)
        return out

    def read_picture_into(self, slot, size, pad=0, threads=4):
        """vvr_read_picture: the finished picture in `slot` (luma size `size`) into arrays whose rows are `pad` samples longer than the picture's
        (a decoder's own buffers have margins); the caller has waited for the picture.  -> list of planes (views without the padding)"""
        ncomp = 3 if self.chroma_format else 1
        arrs = [np.full((size[1] >> (1 if c else 0), (size[0] >> (1 if c else 0)) + pad), 0xffff, np.uint16) for c in range(ncomp)]
        dst = (C.c_void_p * 3)(*[a.ctypes.data for a in arrs] + [None] * (3 - ncomp))
        strides = (C.c_size_t * 3)(*[a.shape[1] for a in arrs] + [0] * (3 - ncomp))
        self._check(self.L.vvr_read_picture(self.ctx, slot, dst, strides, threads))
        for c, a in enumerate(arrs):
            assert pad == 0 or (a[:, a.shape[1] - pad:] == 0xffff).all(), "vvr_read_picture wrote outside the picture"
        return [a[:, :a.shape[1] - pad] if pad else a for a in arrs]

    def picture_hash(self, slot, method=0):
        """decoded picture hash (0 MD5, 1 CRC, 2 checksum): list of per-component digests (bytes)"""
        buf = (C.c_uint8 * 48)()
        n = C.c_int()
        self._check(self.L.vvr_picture_hash(self.ctx, slot, method, buf, C.byref(n)))
        return [bytes(buf[k * n.value:(k + 1) * n.value]) for k in range(3 if self.chroma_format else 1)]

    def set_film_grain(self, bank):
        """the film grain bank read_output(grain=True) applies: None, an abi.FilmGrainBank, or a dict of its fields as arrays (comp_present,
        shift, scale_lut, pattern_lut, pattern; see abi.film_grain_bank).  Does not touch the seed chain."""
        if bank is None:
            self._check(self.L.vvr_set_film_grain(self.ctx, None))
            return
        if not isinstance(bank, abi.FilmGrainBank):
            bank = abi.film_grain_bank(**bank)
        self._check(self.L.vvr_set_film_grain(self.ctx, C.addressof(bank)))

    def set_film_grain_seed(self, seed):
        """the state of the film grain's seed chain (FilmGrain::set_seed; a context starts at 0xdeadbeef)"""
        self._check(self.L.vvr_set_film_grain_seed(self.ctx, seed & 0xffffffff))

    def set_output_colour(self, matrix, full_range=False):
        """the colour description the "rgb8" / "rgb16" / "rgbf16" formats of output_submit convert with (vvr_set_output_colour): H.273
        matrix_coefficients 1 (BT.709), 5 or 6 (BT.601) or 9 (BT.2020 non-constant luminance) and video_full_range_flag.  A request takes the
        value that is set when it is submitted."""
        self._check(self.L.vvr_set_output_colour(self.ctx, int(matrix), 1 if full_range else 0))

    def set_output_narrowing(self, mode, phase=0):
        """how the byte-per-sample Y'CbCr formats of output_submit ("planar8", "nv12", "yuv444p8", "yuv422p8", "uyvy", "yuy2") leave a context of
        9 or 10 bits (vvr_set_output_narrowing, the arithmetic: vvr.h): 0 / "refuse" (a new context: such a request is refused), 1 / "truncate"
        (v >> s), 2 / "round", 3 / "dither" (ordered, a 2 x 2 cell; phase 0 .. 3 moves it by a column and / or a row - nothing advances it).
        The planes are uint8 arrays or tensors of the shapes the formats have in an 8-bit context (abi.output_plane_shapes), `into=` included.  A
        request takes the value that is set when it is submitted; 8-bit contexts and every other format ignore it."""
        if isinstance(mode, str):
            if mode not in abi.NARROW_MODES:
                raise ValueError("set_output_narrowing: mode is 0 .. 3 or one of %s" % ", ".join(abi.NARROW_MODES))
            mode = abi.NARROW_MODES[mode]
        self._check(self.L.vvr_set_output_narrowing(self.ctx, int(mode), int(phase)))

    def set_output_resampling(self, filter):
        """the filter output_submit(size=...) resamples with (vvr_set_output_resampling, the arithmetic: vvr.h): None (a new context: the
        reference's DCTIF, within 1/8 .. 8 times the window), "area", "triangle" (torch's antialiased "bilinear", PIL's BILINEAR) or "cubic"
        (torch's antialiased "bicubic", PIL's BICUBIC) - antialiased, support scaled by the ratio, accepted within 1/64 .. 8 times the window
        in every plane, for every format and destination.  A request takes the value that is set when it is submitted; read_output(size=...),
        the comparisons under set_compare_scaling, statistics and hashes do not look at it."""
        if filter is None or isinstance(filter, str):
            if filter not in abi.RESAMPLE_FILTERS:
                raise ValueError("set_output_resampling: filter is None, 0 .. 3 or one of %s" % ", ".join(k for k in abi.RESAMPLE_FILTERS if k))
            filter = abi.RESAMPLE_FILTERS[filter]
        self._check(self.L.vvr_set_output_resampling(self.ctx, int(filter)))

    def set_compare_scaling(self, size=None, collocated=(True, False)):
        """a reference of another size than the window for compare(), ssim(), msssim() and xpsnr() (vvr_set_compare_scaling, the definition:
        vvr.h): size = (w, h) in luma samples - the window is rescaled to it on the device, exactly as read_output(size=...) delivers it, and
        measured against a reference of that size; result arrays, maps and XPSNR's prev planes are of that size too.  None: off (a new
        context).  collocated: (horizontally, vertically), the chroma phase as read_output takes it.  A slot number as `ref` is refused
        while scaling is on.  A request takes the value that is set when it is submitted."""
        w, h = (0, 0) if size is None else (int(size[0]), int(size[1]))
        self._check(self.L.vvr_set_compare_scaling(self.ctx, w, h, (1 if collocated[0] else 0) | (2 if collocated[1] else 0)))
        self._compare_scaling = (w, h) if w or h else None

    def _measured(self, win):
        """the window as compare(), ssim(), msssim() and xpsnr() measure it: of the size of set_compare_scaling when that is on"""
        return win if self._compare_scaling is None else (0, 0) + self._compare_scaling

    def set_output_normalisation(self, mean=None, std=None):
        """the per-channel mean and standard deviation the "rgbf32" format of output_submit applies (vvr_set_output_normalisation): three floats
        each for R, G, B, in units of full scale (0 .. 1) - out = v / (M * std) - mean / std in two float32 roundings (vvr.h); None: none.  A
        request takes the value that is set when it is submitted; every other format ignores it."""
        if mean is None and std is None:
            self._check(self.L.vvr_set_output_normalisation(self.ctx, None, None))
            return
        m = None if mean is None else (C.c_float * 3)(*[float(v) for v in mean])
        s = None if std is None else (C.c_float * 3)(*[float(v) for v in std])
        self._check(self.L.vvr_set_output_normalisation(self.ctx, m, s))

    def set_output_transform(self, t):
        """the colour transform the "rgb8" / "rgb16" / "rgbf16" formats of output_submit run between the Y'CbCr matrix and the store
        (vvr_set_output_transform): None (none), an abi.OutputTransform (vvdec_amd.output_transform( ... ) makes the standard ones) or a tuple
        (lin, m, enc) of arrays (abi.output_transform).  Under a transform "rgb16" is full-scale 16 bits.  A request takes the transform that is
        set when it is submitted."""
        if t is None:
            self._check(self.L.vvr_set_output_transform(self.ctx, None))
            return
        if not isinstance(t, abi.OutputTransform):
            t = abi.output_transform(*t)
        self._check(self.L.vvr_set_output_transform(self.ctx, C.addressof(t)))

    def set_output_lut3d(self, lut):
        """the 3-D LUT the RGB formats of output_submit run last before the store, behind the transform if one is set (vvr_set_output_lut3d): None
        (none) or (n, nodes) - n 17, 33 or 65, nodes n^3 x 3 uint16 values in .cube order, as vvdec_amd.output_lut3d( ... ) and
        vvdec_amd.read_cube( path ) give them.  Under a LUT "rgb16" is full-scale 16 bits.  A request takes the LUT that is set when it is submitted."""
        if lut is None:
            self._check(self.L.vvr_set_output_lut3d(self.ctx, 0, None))
            return
        n, nodes = lut
        a = abi.lut3d_nodes(n, nodes)
        self._check(self.L.vvr_set_output_lut3d(self.ctx, int(n), a.ctypes.data))      # (copied inside the call)

    def read_output(self, slot, window=None, bytes_per_sample=2, size=None, collocated=(True, False), grain=False):
        """the picture as the application gets it: conformance window (x, y, w, h in luma samples, even) applied, 8- or 16-bit samples.
        size: (width, height) in luma samples to rescale the window to on the device, as vvdec::rescalePlane does (chroma planes get size >> 1,
        vvdecapp's width / chromaSubX); collocated: horizontal, vertical chroma sample position (vvdecapp's 4:2:0 default: True, False).
        grain: film grain of the bank set with set_film_grain added on the device, one frame of the seed chain (vvr_read_output_grain)"""
        x, y, w, h = window or (0, 0, self.width, self.height)
        if grain:
            if size is not None:
                raise ValueError("read_output: grain and size together are not supported (the reference grains before it rescales)")
            nc = 3 if self.chroma_format else 1
            out = [np.zeros((h >> (1 if c else 0), w >> (1 if c else 0)), np.uint8 if bytes_per_sample == 1 else np.uint16) for c in range(nc)]
            ptrs = (C.c_void_p * 3)(*[out[c].ctypes.data if c < nc else None for c in range(3)])
            strides = (C.c_size_t * 3)(*[out[c].strides[0] if c < nc else 0 for c in range(3)])
            self._check(self.L.vvr_read_output_grain(self.ctx, slot, x, y, w, h, bytes_per_sample, ptrs, strides))
            return out
        out = []
        for c in range(3 if self.chroma_format else 1):
            s = 1 if c else 0
            ow, oh = (w, h) if size is None else size
            a = np.zeros((oh >> s, ow >> s), np.uint8 if bytes_per_sample == 1 else np.uint16)
            if size is None:
                self._check(self.L.vvr_read_output(self.ctx, slot, c, x >> s, y >> s, w >> s, h >> s, bytes_per_sample, a.ctypes.data, a.strides[0]))
            else:
                self._check(self.L.vvr_read_output_scaled(self.ctx, slot, c, x >> s, y >> s, w >> s, h >> s, ow >> s, oh >> s,
                                                          int(bool(collocated[0])) | int(bool(collocated[1])) << 1, bytes_per_sample, a.ctypes.data, a.strides[0]))
            out.append(a)
        return out

    # -- output queue: requests ordered behind their picture on the device; nothing here drains the context
    def output_submit(self, slot, job=None, window=None, fmt="planar16", size=None, collocated=(True, False), grain=False, pinned=False, blocking=True, into=None):
        """vvr_output_submit: the window of `slot` (as `job` leaves it; None: as all work submitted so far leaves it) in the application's form ->
        ticket, or None when blocking=False and the job has not been handed to the device yet.  fmt: "planar16", "planar8", "packed10"
        (vvdecapp --pyuv: four samples in five bytes), "nv12" or "p010" (two planes: luma, interleaved CbCr; p010: sample << (16 - bit depth);
        the byte formats - "planar8", "nv12", "yuv444p8", "yuv422p8", "uyvy", "yuy2" - in a context of 9 or 10 bits: set_output_narrowing),
        "rgb8", "rgb16" or "rgbf16" (three planes R, G, B at the luma size, converted on the device with the matrix of set_output_colour: vvr.h);
        "rgbf32" (the three planes as float32 with set_output_normalisation applied), "rgba8", "bgra8", "rgb24", "bgr24", "rgb10a2" or "rgba16f"
        (one plane of interleaved pixels: abi.output_plane_shapes); "yuv444p8", "yuv444p16" (Y, Cb, Cr at the luma size), "yuv422p8", "yuv422p16"
        (Y, and Cb, Cr of w >> 1 samples on every luma row), "uyvy", "yuy2", "y210", "v210" (packed 4:2:2, one plane) or "y410" (packed 4:4:4,
        one plane): Y'CbCr with the chroma upsampled on the device by the filter of the RGB formats, no colour description needed (vvr.h);
        size, collocated, grain as read_output - and grain with size is the reference's chain,
        grain first, then the rescale of the grained frame.  pinned: the planes are allocated in memory of the context that the device writes
        directly (vvr_host_alloc) - they belong to the context and are views valid until close().
        into: the destination planes as 2-D torch tensors on the context's device (row-major, any row stride, element size that of the
        format: abi.output_plane_shapes): the device writes them, nothing crosses PCIe; they are registered with the context for the life of
        the request and output_wait returns them.  The tensors must be idle now and stay untouched until the request has completed
        (output_wait, output_test, or output_stream_wait on the stream that uses them).  At most 8 requests in flight (VvrError).
        The planar RGB formats also take one 3-D tensor of shape (3, h, w) whose last dimension is contiguous (planes and rows may be padded or
        sliced) - float32 for "rgbf32"; the interleaved formats "rgba8", "bgra8", "rgb24", "bgr24" (uint8) and "rgba16f" (float16) one tensor of
        shape (h, w, C) with stride(2) == 1 and stride(1) == C at any row stride, "rgb10a2" one (h, w) tensor of int32; output_wait returns
        that tensor.  "yuv444p8" / "yuv444p16" take a (3, h, w) tensor like planar RGB, "yuv422p8" / "yuv422p16" a list of three 2-D tensors, the
        packed Y'CbCr formats one 2-D tensor of the plane's shape and element size (abi.output_plane_shapes; uint32 planes as int32), which
        output_wait returns.
        Ask for a picture's output before the next picture into its slot is submitted: that picture then waits for the request on the device."""
        win = tuple(window or (0, 0, self.width, self.height))
        shapes, dt = abi.output_plane_shapes(win, fmt, size, 3 if self.chroma_format else 1)
        registered = []
        whole = None
        if into is not None:
            inter = abi.OUT_INTERLEAVED.get(fmt) if isinstance(fmt, str) else None
            if inter is not None and hasattr(into, "dim"):      # one tensor of pixels: (h, w, C), or (h, w) of 4-byte elements for rgb10a2
                h, n = shapes[0]
                ok = (tuple(into.shape) == (h, n) and into.element_size() == 4) if fmt == "rgb10a2" else \
                     (into.dim() == 3 and tuple(into.shape) == (h, n // inter, inter) and into.stride(2) == 1 and into.stride(1) == inter)
                if not ok or min(into.stride()) < 0:
                    raise ValueError("output_submit: %s takes one tensor of shape %r" % (fmt, (h, n) if fmt == "rgb10a2" else (h, n // inter, inter)))
                whole = into
                planes = [into if into.dim() == 2 else into.as_strided((h, n), (into.stride(0), 1))]      # (the plane the request sees: rows of w * C elements)
            elif fmt in abi.OUT_YUV_PACKED and hasattr(into, "dim"):      # one 2-D tensor: the packed plane
                if into.dim() != 2 or min(into.stride()) < 0:
                    raise ValueError("output_submit: %s takes one 2-D tensor of shape %r" % (fmt, tuple(shapes[0])))
                whole = into
                planes = [into]
            elif hasattr(into, "dim") and into.dim() == 3:      # (3, h, w): its planes, registered as one range
                if len(shapes) != 3 or len(set(shapes)) != 1 or into.shape[0] != 3 or min(into.stride()) < 0:
                    raise ValueError("output_submit: a 3-D tensor serves the planar RGB formats and 4:4:4 Y'CbCr, as (3, h, w)")
                whole = into
                planes = list(into)
            else:
                planes = list(into)
            if len(planes) != len(shapes):
                raise ValueError("output_submit: %s needs %d planes" % (fmt, len(shapes)))
            for t, shape in zip(planes, shapes):
                if not t.is_cuda or t.device.index != self.cfg.device or t.dim() != 2 or tuple(t.shape) != tuple(shape) or t.element_size() != np.dtype(dt).itemsize or (t.shape[1] > 1 and t.stride(1) != 1):
                    raise ValueError("output_submit: into needs row-major 2-D tensors on the context's device, here of shape %r and %d-byte elements" % (shape, np.dtype(dt).itemsize))
            try:
                for t in [whole] if whole is not None else planes:
                    ptr, n = t.data_ptr(), (sum((d - 1) * st for d, st in zip(t.shape, t.stride())) + 1) * t.element_size()
                    if any(a <= ptr and ptr + n <= a + m for a, m in self._dev):
                        continue
                    self._check(self.L.vvr_device_register(self.ctx, ptr, n))
                    registered.append(ptr)
            except VvrError:
                for ptr in registered:
                    self.L.vvr_device_unregister(self.ctx, ptr)
                raise
        else:
            planes = [self.host_array(r * n, dt).reshape(r, n) if pinned else np.zeros((r, n), dt) for r, n in shapes]
        req = abi.output_request(slot, job, win, fmt, size, collocated, grain, blocking, planes)
        ticket = self.L.vvr_output_submit(self.ctx, C.byref(req))
        if ticket < 0 or ticket == abi.VVR_NOT_READY:
            for ptr in registered:
                self.L.vvr_device_unregister(self.ctx, ptr)
        self._check(ticket)
        if not blocking and ticket == abi.VVR_NOT_READY:
            return None
        self._out[ticket] = planes if whole is None else whole
        self._reg[ticket] = registered
        return ticket

    def output_submit_batch(self, slot, origins, window_size, fmt, job=None, size=None, collocated=(True, False), pinned=False, blocking=True, into=None):
        """vvr_output_submit_batch: the regions of `slot` of window_size = (w, h) at `origins` ((x, y) pairs, up to 256) as one request, one ticket
        and one launch per stage -> ticket, or None when blocking=False and the job has not been handed to the device yet.  Region i gets exactly
        what output_submit(slot, window=(x_i, y_i, w, h), fmt=fmt, size=size, collocated=collocated) gives.  fmt: one of abi.OUT_BATCH_FORMATS,
        the ten R'G'B' formats.  output_wait returns the regions stacked on a leading axis: (N, 3, H, W) for the planar formats, (N, H, W, C)
        for the interleaved ones, (N, H, W) words for "rgb10a2" - a numpy array (pinned: in memory of the context that the device writes
        directly), or the tensor given as
        into: a contiguous torch tensor of that shape on the context's device (rgb10a2: int32), written by the device and registered with the
        context for the life of the request, as output_submit does it; it must be idle now and stay untouched until the request has completed."""
        origins = [tuple(int(v) for v in o) for o in origins]
        n, (w, h) = len(origins), window_size
        shapes, dt = abi.output_plane_shapes((0, 0, w, h), fmt, size, 3 if self.chroma_format else 1)
        if fmt not in abi.OUT_BATCH_FORMATS:
            raise ValueError("output_submit_batch: fmt is one of %r" % (abi.OUT_BATCH_FORMATS,))
        rows, per_row = shapes[0]
        inter = abi.OUT_INTERLEAVED.get(fmt)
        shape = (n, 3, rows, per_row) if inter is None else (n, rows, per_row) if fmt == "rgb10a2" else (n, rows, per_row // inter, inter)
        item = np.dtype(dt).itemsize
        plane_bytes, region_bytes = rows * per_row * item, len(shapes) * rows * per_row * item
        registered = []
        if into is not None:
            if not hasattr(into, "is_cuda") or not into.is_cuda or into.device.index != self.cfg.device or tuple(into.shape) != shape or into.element_size() != item or not into.is_contiguous():
                raise ValueError("output_submit_batch: into is a contiguous tensor on the context's device of shape %r and %d-byte elements" % (shape, item))
            out, base = into, into.data_ptr()
            if n and not any(a <= base and base + n * region_bytes <= a + m for a, m in self._dev):
                self._check(self.L.vvr_device_register(self.ctx, base, n * region_bytes))
                registered.append(base)
        else:
            out = self.host_array(max(1, n * region_bytes // item), dt)[:n * region_bytes // item].reshape(shape) if pinned else np.zeros(shape, dt)
            base = out.ctypes.data
        req = abi.OutputRequest()
        req.struct_size, req.slot, req.job = C.sizeof(abi.OutputRequest), slot, -1 if job is None else job
        req.x, req.y, req.w, req.h = 0, 0, w, h
        req.out_w, req.out_h = size or (0, 0)
        req.collocated = int(bool(collocated[0])) | int(bool(collocated[1])) << 1
        req.format, req.grain, req.blocking = abi.OUT_FORMATS[fmt], 0, 1 if blocking else 0
        for k in range(len(shapes)):
            req.dst[k], req.dst_stride_bytes[k] = base + k * plane_bytes, per_row * item
        batch, keep = abi.output_batch(origins, [region_bytes] * len(shapes))
        ticket = self.L.vvr_output_submit_batch(self.ctx, C.byref(req), C.byref(batch))
        if ticket < 0 or ticket == abi.VVR_NOT_READY:
            for ptr in registered:
                self.L.vvr_device_unregister(self.ctx, ptr)
        self._check(ticket)
        if not blocking and ticket == abi.VVR_NOT_READY:
            return None
        self._out[ticket] = out
        self._reg[ticket] = registered
        return ticket

    def output_stream_wait(self, ticket, stream=None):
        """vvr_output_stream_wait: `stream` (a torch.cuda.Stream, or a hipStream_t as an int; None: torch's current stream) waits on the device
        for the completion of the request; the host does not wait.  The ticket stays for output_wait."""
        if stream is None:
            import torch
            stream = torch.cuda.current_stream(self.cfg.device)
        self._check(self.L.vvr_output_stream_wait(self.ctx, ticket, getattr(stream, "cuda_stream", stream)))

    def output_test(self, ticket):
        """vvr_output_test: True when output_wait(ticket) returns at once; raises if the request (or its picture) failed"""
        rc = self.L.vvr_output_test(self.ctx, ticket)
        if rc == abi.VVR_NOT_READY:
            return False
        self._check(rc)
        return True

    def output_wait(self, ticket):
        """vvr_output_wait: blocks for this request only and retires the ticket -> list of planes (packed10: uint8 arrays of (rows, w / 4 * 5); the
        tensors - or the one (3, h, w) tensor - of output_submit(into=...), which are unregistered here)"""
        try:
            self._check(self.L.vvr_output_wait(self.ctx, ticket))
            return self._out[ticket]
        finally:
            self._out.pop(ticket, None)
            for ptr in self._reg.pop(ticket, []):
                self.L.vvr_device_unregister(self.ctx, ptr)

    def hash_submit(self, slot, job=None, method=0, expected=None, blocking=True):
        """vvr_hash_submit: the decoded picture hash of `slot` (as `job` leaves it; None: as all work submitted so far leaves it) as a request of
        the output queue -> ticket, or None when blocking=False and the job has not been handed to the device yet.  method: 0 MD5, 1 CRC,
        2 checksum (CRC and checksum are finished on the device; for MD5 the picture's bytes come to the host and hash_wait hashes them).
        expected: the SEI's digests (a list of bytes per component, or their concatenation) to compare with.  The ticket shares the 8 entries of
        output_submit; output_test and output_stream_wait take it.  Nothing here drains the context (picture_hash does)."""
        nc, n = 3 if self.chroma_format else 1, abi.HASH_LEN[method]
        r = abi.HashRequest()
        r.struct_size, r.slot, r.job, r.method, r.blocking = C.sizeof(abi.HashRequest), slot, -1 if job is None else job, method, 1 if blocking else 0
        digest, mismatch, want = (C.c_uint8 * (nc * n))(), C.c_uint32(0xffffffff), None
        r.digest = C.addressof(digest)
        if expected is not None:
            raw = expected if isinstance(expected, (bytes, bytearray)) else b"".join(expected)
            if len(raw) != nc * n:
                raise ValueError("hash_submit: expected needs %d digests of %d bytes" % (nc, n))
            want = (C.c_uint8 * len(raw)).from_buffer_copy(raw)
            r.expected, r.mismatch = C.addressof(want), C.addressof(mismatch)
        ticket = self._check(self.L.vvr_hash_submit(self.ctx, C.byref(r)))
        if not blocking and ticket == abi.VVR_NOT_READY:
            return None
        self._out[ticket] = (digest, mismatch if expected is not None else None, nc, n)
        return ticket

    def hash_wait(self, ticket):
        """vvr_output_wait for a ticket of hash_submit -> (list of per-component digests as bytes, mismatch mask or None when nothing was
        expected): bit c of the mask is set when component c differs from the expected digest, 0 means the picture is verified"""
        digest, mismatch, nc, n = self.output_wait(ticket)
        return [bytes(digest[k * n:(k + 1) * n]) for k in range(nc)], None if mismatch is None else mismatch.value

    def stats_submit(self, slot, job=None, window=None, mode="rgb", collocated=(True, False), blocking=True):
        """vvr_stats_submit: light-level statistics of the window of `slot` (as `job` leaves it; None: as all work submitted so far leaves it),
        reduced on the device -> ticket, or None when blocking=False and the job has not been handed to the device yet.  mode "rgb": the luma
        histogram, the histogram of max( R, G, B ) and the channels' extremes of the coded R'G'B' (the matrix of set_output_colour at the
        context's bit depth; transform, LUT and normalisation are ignored); "luma": the luma histogram alone, in any context.  The ticket
        shares the 8 entries of output_submit; output_test and output_stream_wait take it.  Nothing here drains the context."""
        raw = abi.FrameStats()
        req = abi.stats_request(slot, job, tuple(window or (0, 0, self.width, self.height)), mode, collocated, blocking, raw)
        ticket = self._check(self.L.vvr_stats_submit(self.ctx, C.byref(req)))
        if not blocking and ticket == abi.VVR_NOT_READY:
            return None
        self._out[ticket] = raw
        return ticket

    def stats_wait(self, ticket):
        """vvr_output_wait for a ticket of stats_submit -> FrameStats (numpy views hist_y, hist_maxrgb, max_c, min_c; vvdec_amd.light_level
        turns it into light levels)"""
        return FrameStats(self.output_wait(ticket))

    def _against_reference(self, what, slot, ref, win, job, request, submit, raw, blocks, prev=None):
        """the part compare(), ssim(), msssim() and xpsnr() share: the reference looked at (a slot number, numpy planes, or torch tensors on the
        device, which are registered with the context for the call's duration), the request made by `request`, submitted with `submit` and
        waited for; `raw` and `blocks` are written.  prev: a list of further luma planes of the window's size (xpsnr), looked at alike and
        replaced in place by what the request is to point to"""
        nc = 3 if self.chroma_format else 1
        registered = []
        size = self._measured(win)      # (the window's size, or the size it is rescaled to)
        if prev:
            if any(tuple(p.shape) != (size[3], size[2]) for p in prev):
                raise ValueError("%s: prev planes are luma planes of the window's size, %r" % (what, (size[3], size[2])))
            if all(hasattr(p, "data_ptr") for p in prev):
                if any(not p.is_cuda or p.device.index != self.cfg.device or p.element_size() not in (1, 2) or (p.shape[1] > 1 and p.stride(1) != 1) or p.stride(0) < 0 for p in prev):
                    raise ValueError(what + ": prev tensors are row-major 2-D tensors of 1- or 2-byte elements on the context's device")
            else:
                prev[:] = [np.asarray(p) for p in prev]
                if any(p.dtype not in (np.uint8, np.uint16) for p in prev):
                    raise ValueError(what + ": prev planes are uint8 or uint16 arrays")
                prev[:] = [p if p.strides[1] == p.itemsize and p.strides[0] > 0 else np.ascontiguousarray(p) for p in prev]
        if not isinstance(ref, int):
            ref = list(ref)[:nc]
            shapes = [(size[3] >> (1 if c else 0), size[2] >> (1 if c else 0)) for c in range(nc)]
            if len(ref) != nc or any(tuple(p.shape) != s for p, s in zip(ref, shapes)):
                raise ValueError("%s: the reference needs %d planes of the window's size, %r" % (what, nc, shapes))
            if all(hasattr(p, "data_ptr") for p in ref):
                if any(not p.is_cuda or p.device.index != self.cfg.device or p.element_size() not in (1, 2) or p.element_size() != ref[0].element_size() or
                       (p.shape[1] > 1 and p.stride(1) != 1) or p.stride(0) < 0 for p in ref):
                    raise ValueError(what + ": reference tensors are row-major 2-D tensors of 1- or 2-byte elements on the context's device")
            else:
                ref = [np.asarray(p) for p in ref]
                if ref[0].dtype not in (np.uint8, np.uint16) or any(p.dtype != ref[0].dtype for p in ref):
                    raise ValueError(what + ": reference planes are uint8 or uint16 arrays")
                ref = [p if p.strides[1] == p.itemsize and p.strides[0] > 0 else np.ascontiguousarray(p) for p in ref]
        try:
            tensors = [t for t in ([] if isinstance(ref, int) else ref) + list(prev or ()) if hasattr(t, "data_ptr")]
            if tensors:
                for t in tensors:
                    ptr, n = t.data_ptr(), (sum((d - 1) * st for d, st in zip(t.shape, t.stride())) + 1) * t.element_size()
                    if any(a <= ptr and ptr + n <= a + m for a, m in self._dev) or ptr in registered:
                        continue
                    self._check(self.L.vvr_device_register(self.ctx, ptr, n))
                    registered.append(ptr)
            req = request(slot, job, win, ref, raw, blocks)
            ticket = self._check(submit(self.ctx, C.byref(req)))
            self._check(self.L.vvr_output_wait(self.ctx, ticket))
        finally:
            for ptr in registered:
                self.L.vvr_device_unregister(self.ctx, ptr)

    def compare(self, slot, ref, window=None, job=None, with_map=False):
        """vvr_compare_submit and vvr_output_wait: the window of `slot` (as `job` leaves it; None: as all work submitted so far leaves it)
        compared sample by sample with a reference frame, reduced on the device -> dict of per-component lists (width, height, samples,
        differing, sse, sad, max_abs, first: (x, y) of the first differing sample in raster order or None), bit_depth, num_components, `raw`
        (the abi.FrameCompare psnr takes) and, with_map, `map`: a uint32 array with the differing samples of every block of 64 x 64 luma
        samples.  ref: a slot number (the same window of that slot), or the window's planes as numpy arrays (uint8 or uint16; copied during
        the call) or as 2-D torch tensors on the context's device (read in place: registered with the context for the call's duration;
        they must be idle).  Nothing here drains the context."""
        win = tuple(window or (0, 0, self.width, self.height))
        nc = 3 if self.chroma_format else 1
        raw = abi.FrameCompare()
        blocks = np.zeros(abi.compare_map_shape(self._measured(win)), np.uint32) if with_map else None
        self._against_reference("compare", slot, ref, win, job, abi.compare_request, self.L.vvr_compare_submit, raw, blocks)
        out = dict(raw=raw, bit_depth=raw.bit_depth, num_components=raw.num_components)
        for name in ("width", "height", "samples", "differing", "sse", "sad", "max_abs"):
            out[name] = [int(v) for v in getattr(raw, name)][:nc]
        out["first"] = [(raw.first_x[c], raw.first_y[c]) if raw.differing[c] else None for c in range(nc)]
        if with_map:
            out["map"] = blocks
        return out

    def psnr(self, compared, peak=0.):
        """vvr_compare_psnr: PSNR in dB from the sums of compare() (its dict, or an abi.FrameCompare) -> [Y, Cb, Cr, all components together];
        peak <= 0: 2^bit depth - 1; inf where nothing differs, 0 for the components a 4:0:0 context lacks"""
        out = (C.c_double * 4)()
        raw = compared["raw"] if isinstance(compared, dict) else compared
        if self.L.vvr_compare_psnr(C.byref(raw), float(peak), out) != abi.VVR_OK:
            raise VvrError("vvr_compare_psnr: a result of compare() at 8 to 10 bits")
        return list(out)

    def ssim(self, slot, ref, window=None, job=None, with_map=False):
        """vvr_ssim_submit and vvr_output_wait: SSIM of the window of `slot` against a reference frame, reduced on the device (8 x 8 windows at a
        stride of 4, integers defined in vvr.h) -> dict: `ssim` [Y, Cb, Cr, all components together] as floats (vvr_compare_ssim), per-component
        lists sum, windows, min (Q24 integers) and min_at ((x, y) of the first window in raster order that has the smallest value, or None),
        width, height, bit_depth, num_components, `raw` (the abi.FrameSsim) and, with_map, `map`: an int32 array with the smallest value of every
        block of 64 x 64 luma samples (0x7fffffff: no window starts there).  slot, ref, window, job: as compare()."""
        win = tuple(window or (0, 0, self.width, self.height))
        nc = 3 if self.chroma_format else 1
        raw = abi.FrameSsim()
        blocks = np.zeros(abi.ssim_map_shape(self._measured(win)), np.int32) if with_map else None
        self._against_reference("ssim", slot, ref, win, job, abi.ssim_request, self.L.vvr_ssim_submit, raw, blocks)
        mean = (C.c_double * 4)()
        if self.L.vvr_compare_ssim(C.byref(raw), mean) != abi.VVR_OK:
            raise VvrError("vvr_compare_ssim: a result of vvr_ssim_submit at 8 to 10 bits")
        out = dict(raw=raw, bit_depth=raw.bit_depth, num_components=raw.num_components, ssim=list(mean))
        for name in ("width", "height", "sum", "windows", "min"):
            out[name] = [int(v) for v in getattr(raw, name)][:nc]
        out["min_at"] = [(raw.min_x[c], raw.min_y[c]) if raw.windows[c] else None for c in range(nc)]
        if with_map:
            out["map"] = blocks
        return out

    def msssim(self, slot, ref, window=None, job=None, scales=5, weights=None):
        """vvr_msssim_submit and vvr_output_wait: MS-SSIM of the window of `slot` against a reference frame over `scales` levels (1 .. 5), the
        pyramid of 2 x 2 rounded means built and every level reduced on the device (integers defined in vvr.h) -> dict: `msssim` [Y, Cb, Cr,
        all components together] as floats (vvr_compare_msssim with `weights`: None, Wang et al.'s normalised to the scales taken, or `scales`
        non-negative numbers), per-level lists of per-component lists width, height, windows, sum_cs, sum_v (Q24 sums), scales, bit_depth,
        num_components, `raw` (the abi.FrameMsssim).  slot, ref, window, job: as compare()."""
        win = tuple(window or (0, 0, self.width, self.height))
        nc = 3 if self.chroma_format else 1
        raw = abi.FrameMsssim()
        self._against_reference("msssim", slot, ref, win, job, lambda s, j, w, r, res, _: abi.msssim_request(s, j, w, r, res, scales), self.L.vvr_msssim_submit, raw, None)
        if weights is not None:
            if len(weights) != scales:
                raise ValueError("msssim: %d weights for %d scales" % (len(weights), scales))
            weights = (C.c_double * scales)(*weights)
        value = (C.c_double * 4)()
        if self.L.vvr_compare_msssim(C.byref(raw), weights, value) != abi.VVR_OK:
            raise VvrError("vvr_compare_msssim: a result of vvr_msssim_submit, and weights that are finite and not negative")
        out = dict(raw=raw, bit_depth=raw.bit_depth, num_components=raw.num_components, scales=raw.scales, msssim=list(value))
        for name in ("width", "height", "windows", "sum_cs", "sum_v"):
            out[name] = [[int(v) for v in getattr(raw, name)[k]][:nc] for k in range(raw.scales)]
        return out

    def xpsnr(self, slot, ref, prev=(), window=None, job=None, block=0, filter=0, a_pic=0, peak=0, with_blocks=False):
        """vvr_xpsnr_submit and vvr_output_wait: XPSNR of the window of `slot` against a reference frame, the block-wise sums taken on the device
        (integers defined in vvr.h) -> dict: `xpsnr` [Y, Cb, Cr, all components together] as floats (vvr_compare_xpsnr with a_pic and peak; 0:
        its defaults), the totals sse (per component), act_spatial, act_temporal, count, the geometry block, filter (both resolved), blocks_x,
        blocks_y, temporal, width, height, samples, bit_depth, num_components, `raw` (the abi.FrameXpsnr) and, with_blocks, `blocks`: a
        structured array (np.dtype(abi.XPSNR_BLOCK_FIELDS)) of blocks_y x blocks_x records.  prev: the luma planes of the reference one and two frames
        earlier (0, 1 or 2 of them: `temporal`), of the window's size, numpy arrays or tensors as `ref` is - with a reference given by
        pointer, of the same kind and element size.  slot, ref, window, job: as compare()."""
        win = tuple(window or (0, 0, self.width, self.height))
        nc = 3 if self.chroma_format else 1
        prev = list(prev)
        if len(prev) > 2:
            raise ValueError("xpsnr: at most two prev planes")
        shape = abi.xpsnr_blocks(self._measured(win)[2], self._measured(win)[3], block)
        if shape is None:
            raise ValueError("xpsnr: a window of at least 8 x 8, a block that is 0 or a multiple of 4, at most %d blocks" % abi.XPSNR_MAX_BLOCKS)
        raw = abi.FrameXpsnr()
        records = np.zeros((shape[2], shape[1]), np.dtype(abi.XPSNR_BLOCK_FIELDS))
        self._against_reference("xpsnr", slot, ref, win, job, lambda s, j, w, r, res, b: abi.xpsnr_request(s, j, w, r, res, prev, b, block=block, filter=filter),
                                self.L.vvr_xpsnr_submit, raw, records, prev)
        value = (C.c_double * 4)()
        if self.L.vvr_compare_xpsnr(C.byref(raw), records.ctypes.data, float(a_pic), float(peak), value) != abi.VVR_OK:
            raise VvrError("vvr_compare_xpsnr: a result of vvr_xpsnr_submit")
        out = dict(raw=raw, xpsnr=list(value), act_spatial=int(raw.act_spatial), act_temporal=int(raw.act_temporal), count=int(raw.count))
        for name in ("bit_depth", "num_components", "temporal", "filter", "block", "blocks_x", "blocks_y"):
            out[name] = int(getattr(raw, name))
        for name in ("width", "height", "samples", "sse"):
            out[name] = [int(v) for v in getattr(raw, name)][:nc]
        if with_blocks:
            out["blocks"] = records
        return out

    def write_picture(self, slot, planes):
        for c, pl in enumerate(planes):
            a = np.ascontiguousarray(pl, dtype=np.uint16)
            assert a.shape == self.plane_shape(c)
            self._check(self.L.vvr_write_plane(self.ctx, slot, c, a.ctypes.data, a.shape[1]))

    @staticmethod
    def new_dpb_tensor(width, height, num_slots, chroma_format=1, device="cuda"):
        """uint8 torch tensor that can hold the DPB of a context (pass its data_ptr() as ext_planes): slot s is the byte range
        [s * slot_bytes, (s + 1) * slot_bytes), which is what vvdec_amd.parallel.PictureParallel broadcasts between ranks"""
        import torch
        cfg = abi.Config()
        cfg.abi_version = abi.VVR_ABI_VERSION
        cfg.max_width, cfg.max_height, cfg.chroma_format = width, height, chroma_format
        nbytes = lib().vvr_slot_bytes(C.byref(cfg)) * num_slots
        return torch.zeros(nbytes, dtype=torch.uint8, device=device)

    def plane_ptr(self, slot, comp):
        return self.L.vvr_plane_ptr(self.ctx, slot, comp)

    def slot_bytes(self):
        return self.L.vvr_slot_bytes(C.byref(self.cfg))

    def plane_layout(self, comp):
        off, st, w, h = C.c_size_t(), C.c_size_t(), C.c_int(), C.c_int()
        self._check(self.L.vvr_plane_layout(self.ctx, comp, C.byref(off), C.byref(st), C.byref(w), C.byref(h)))
        return off.value, st.value, w.value, h.value

    # -- statistics (HIP events around every kernel launch, on the launch stream)
    def enable_stats(self, on=True):
        self._check(self.L.vvr_enable_stats(self.ctx, 1 if on else 0))

    def stats(self):
        arr = (abi.KernelStat * 64)()
        n = self._check(self.L.vvr_get_stats(self.ctx, arr, 64))
        return [dict(name=arr[i].name.decode(), launches=arr[i].launches, total_ms=arr[i].total_ms, algo_bytes=arr[i].algo_bytes) for i in range(n)]
