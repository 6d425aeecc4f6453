"""TEST INFRASTRUCTURE: the reference's own film grain synthesis (vvdec::FilmGrain, source/Lib/FilmGrain, exported by oracle/_ref/libvvref.so, which
links the reference's objects whole with default visibility) on a sequence of operations, in a child process (libvvref.so must not share a process
with the drop-in libvvdec.so: both define the vvdec_* API).

    python tests/film_grain_ref.py <ops.json> <in.npz> <out.npz>

Operations, in order, on one FilmGrain object (what VVDecImpl keeps in m_filmGrainSynth):
  ["fgc", sei]         FilmGrain::updateFGC with a vvdecSEIFilmGrainCharacteristics (sei.h:193-223) built from the dict `sei`; the bank
                       (vvr_film_grain_bank's fields) is read back out of the object: patterns, sLUT, pLUT and the scale shift of its FilmGrainImpl,
                       comp_model_present_flag of its fgs_sei (which updateFGC never clears)
  ["seed", s]          FilmGrain::set_seed( s )
  ["frame", n, bd, cf] frame n of in.npz (f<n>_c<k>, uint16) grained as VVDecImpl::xAddGrain does it (vvdecimpl.cpp:897-956): set_depth,
                       setColorFormat (4:2:0; the reference's 4:0:0 setColorFormat refuses, so 4:0:0 frames keep the default and pass no chroma),
                       prepareBlockSeeds( w, h ), add_grain_line for every row, single-threaded, rows at a padded stride.  The padding beyond
                       each row's end repeats the row's last sample.
sei: dict(model_id, log2_scale_factor, comps=[None or dict(num_model_values, intervals=[[lo, hi, [v0..v5]], ...])] * 3)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF_LIB = os.path.join(HERE, "..", "oracle", "_ref", "libvvref.so")

SYM = dict(ctor="_ZN5vvdec9FilmGrainC1Ev", update="_ZN5vvdec9FilmGrain9updateFGCEP32vvdecSEIFilmGrainCharacteristics",
           seeds="_ZN5vvdec9FilmGrain17prepareBlockSeedsEii", line="_ZN5vvdec9FilmGrain14add_grain_lineEPvS1_S1_ii",
           color="_ZN5vvdec9FilmGrain14setColorFormatE16vvdecColorFormat", seed="_ZN5vvdec9FilmGrain8set_seedEj",
           depth="_ZN5vvdec13FilmGrainImpl9set_depthEi")

# FilmGrainImpl (FilmGrainImpl.h:91-104) after its vptr: int8 pattern[2][9][64][64], uint8 sLUT[3][256], pLUT[3][256], uint8 scale_shift, bs,
# int csubx, csuby
IMPL_PATTERN, IMPL_SLUT, IMPL_PLUT = 8, 8 + 2 * 9 * 4096, 8 + 2 * 9 * 4096 + 768
IMPL_SHIFT, IMPL_BS, IMPL_CSUBX = IMPL_PLUT + 768, IMPL_PLUT + 769, IMPL_PLUT + 772
# FilmGrain (FilmGrain.h:69-78): unique_ptr m_impl, uint32 m_line_rnd, m_line_rnd_up, m_prev_frame_line_rnd_up, vector m_line_seeds, fgs_sei fgs
FG_LINE_RND, FG_FGS = 8, 48


def available():
    return os.path.exists(REF_LIB)


class CompModelIntensityValues(C.Structure):
    _fields_ = [("intensityIntervalLowerBound", C.c_uint8), ("intensityIntervalUpperBound", C.c_uint8), ("compModelValue", C.c_int * 6)]


class CompModel(C.Structure):
    _fields_ = [("presentFlag", C.c_bool), ("numModelValues", C.c_uint8), ("numIntensityIntervals", C.c_uint16), ("intensityValues", CompModelIntensityValues * 256)]


class SEIFilmGrainCharacteristics(C.Structure):
    _fields_ = [("filmGrainCharacteristicsCancelFlag", C.c_bool), ("filmGrainModelId", C.c_uint8), ("separateColourDescriptionPresentFlag", C.c_bool),
                ("filmGrainBitDepthLuma", C.c_uint8), ("filmGrainBitDepthChroma", C.c_uint8), ("filmGrainFullRangeFlag", C.c_bool),
                ("filmGrainColourPrimaries", C.c_uint8), ("filmGrainTransferCharacteristics", C.c_uint8), ("filmGrainMatrixCoeffs", C.c_uint8),
                ("blendingModeId", C.c_uint8), ("log2ScaleFactor", C.c_uint8), ("compModel", CompModel * 3), ("filmGrainCharacteristicsPersistenceFlag", C.c_bool)]


def sei_struct(sei):
    s = SEIFilmGrainCharacteristics()
    s.filmGrainModelId = sei["model_id"]
    s.log2ScaleFactor = sei["log2_scale_factor"]
    s.filmGrainCharacteristicsPersistenceFlag = bool(sei.get("persistence", True))
    for c, comp in enumerate(sei["comps"]):
        if comp is None:
            continue
        cm = s.compModel[c]
        cm.presentFlag = True
        cm.numModelValues = comp["num_model_values"]
        cm.numIntensityIntervals = len(comp["intervals"])
        for k, (lo, hi, vals) in enumerate(comp["intervals"]):
            iv = cm.intensityValues[k]
            iv.intensityIntervalLowerBound, iv.intensityIntervalUpperBound = lo, hi
            for v in range(comp["num_model_values"]):
                iv.compModelValue[v] = vals[v]
    return s


def run(ops, frames, tmpdir, name="fg"):
    """ops as in the module's text, frames: list of lists of uint16 planes -> list of results, one per operation: a bank dict for "fgc", None for
    "seed", the grained planes (uint16) for "frame" """
    jin, nin, nout = (os.path.join(tmpdir, name + ext) for ext in (".ops.json", ".in.npz", ".out.npz"))
    with open(jin, "w") as f:
        json.dump(ops, f)
    np.savez(nin, **{"f%d_c%d" % (n, k): np.ascontiguousarray(p, np.uint16) for n, fr in enumerate(frames) for k, p in enumerate(fr)})
    subprocess.check_call([sys.executable, os.path.abspath(__file__), jin, nin, nout], timeout=1200)
    got = np.load(nout)
    out = []
    for n, op in enumerate(ops):
        if op[0] == "fgc":
            out.append(dict(comp_present=got["o%d_present" % n], shift=int(got["o%d_shift" % n]), scale_lut=got["o%d_slut" % n],
                            pattern_lut=got["o%d_plut" % n], pattern=got["o%d_pattern" % n]))
        elif op[0] == "frame":
            out.append([got["o%d_c%d" % (n, k)] for k in range(len(frames[op[1]]))])
        else:
            out.append(None)
    return out


def random_sei(rng, model_id, n_intervals, log2_scale_factor, chroma=True, absent=None, persistence=True):
    """an FGC SEI: n_intervals intensity intervals per present component with holes between them (a third of the range left out), model values
    in the ranges the models take (frequency cut-offs 2..14, small auto-regressive coefficients), component `absent` not present.  Scale factors
    below 128: the reference's x86 SIMD scale_and_output (FilmGrainImpl_X86_SIMD.h) sign-extends the 8-bit scale where its plain C++ model
    (FilmGrainImpl.cpp:284) and vvr_read_output_grain take it unsigned, so the two agree only there"""
    comps = []
    for c in range(3):
        if c == absent or (c and not chroma):
            comps.append(None)
            continue
        bounds = np.sort(rng.choice(256, 2 * n_intervals, replace=False))
        intervals = []
        for k in range(n_intervals):
            lo, hi = int(bounds[2 * k]), int(bounds[2 * k + 1])
            if k % 3 == 2:
                hi = lo + (hi - lo) // 3          # holes
            if model_id == 0:
                vals = [int(rng.integers(0, 128)), int(rng.integers(2, 15)), int(rng.integers(2, 15)), 0, 0, 0]
            else:
                vals = [int(rng.integers(0, 128)), int(rng.integers(-24, 48)), int(rng.integers(-16, 16)), int(rng.integers(-8, 8)),
                        int(rng.integers(0, 1 << log2_scale_factor)), int(rng.integers(-8, 8))]
            intervals.append([lo, hi, vals])
        comps.append(dict(num_model_values=int(rng.integers(1, 4)) if model_id == 0 else 6, intervals=intervals))
    return dict(model_id=model_id, log2_scale_factor=log2_scale_factor, comps=comps, persistence=persistence)


def grain_picture(rng, W, H, bd, cf):
    """planes of a picture (uint16) with every intensity, rows at the top of the range (10-bit: 1021 - 1023, 8-bit: 255, the clip's ceiling) and at 0"""
    planes = []
    for c in range(3 if cf else 1):
        h, w = (H >> 1, W >> 1) if c else (H, W)
        p = rng.integers(0, 1 << bd, (h, w))
        p[h // 4:h // 4 + 6] = rng.integers((1 << bd) - 3, 1 << bd, (6, w))
        p[h // 2:h // 2 + 3] = 0
        p[:, w // 3:w // 3 + 5] = (1 << bd) - 1
        planes.append(p.astype(np.uint16))
    return planes


def matrix_sequence(bd, cf, seed=1):
    """the case matrix as one sequence of steps on one context: ("fgc", sei), ("seed", s), ("frame", (x, y, w, h), bytes per sample) - windows of
    a 448 x 160 picture at odd (4:0:0) and even offsets, widths 136, 200, 384, 146 (4:2:0 chroma width 1 mod 8) or 145 (1 mod 16) and 129, heights
    that are no multiple of 16, frames of different sizes one after the other, banks of models 0 and 1 with 1, 3 and 8 intervals, holes and an
    absent component, log2_scale_factor 2..7, a new bank mid-sequence (the seed chain goes on) and a seed set mid-sequence; 8-bit: 1- and 2-byte
    output in turn"""
    rng = np.random.default_rng(seed * 100 + bd * 10 + cf)
    odd = 0 if cf else 1
    ch = bool(cf)
    steps = [("fgc", random_sei(rng, 0, 1, 2, ch)),
             ("frame", (0, 0, 136, 64)),
             ("frame", (2 + odd, 6 + odd, 200, 40)),
             ("fgc", random_sei(rng, 1, 3, 5, ch, absent=2 if cf else None)),
             ("frame", (4 + odd, 2, 384, 98)),
             ("frame", (10, 16 + odd, 146 if cf else 145, 50)),
             ("seed", int(rng.integers(0, 1 << 32))),
             ("fgc", random_sei(rng, 0, 8, 7, ch, absent=0 if cf else None)),
             ("frame", (0, 0, 448, 160)),
             ("fgc", random_sei(rng, 1, 8, 3, ch)),
             ("frame", (6, 8 + 2 * odd, 130 if cf else 129, 34)),
             ("fgc", random_sei(rng, 0, 3, 4, ch)),
             ("frame", (40 + odd, 30, 256, 66)),
             ("fgc", random_sei(rng, 1, 1, 6, ch)),
             ("frame", (12, 4, 320, 120))]
    n = 0
    for k, st in enumerate(steps):
        if st[0] == "frame":
            steps[k] = ("frame", st[1], 1 if bd == 8 and n % 2 else 2)
            n += 1
    return grain_picture(rng, 448, 160, bd, cf), steps


def expected(picture, steps, bd, cf, tmpdir, name="fg"):
    """-> the banks of the "fgc" steps and the grained frames of the "frame" steps, in order, by the reference"""
    ops, frames = [], []
    for st in steps:
        if st[0] == "frame":
            x, y, w, h = st[1]
            frames.append([p[y >> (1 if c else 0):(y + h) >> (1 if c else 0), x >> (1 if c else 0):(x + w) >> (1 if c else 0)] for c, p in enumerate(picture)])
            ops.append(["frame", len(frames) - 1, bd, cf])
        else:
            ops.append(list(st))
    res = run(ops, frames, tmpdir, name)
    return [r for op, r in zip(ops, res) if op[0] == "fgc"], [r for op, r in zip(ops, res) if op[0] == "frame"]


def _main(jin, nin, nout):
    ops = json.load(open(jin))
    frames = np.load(nin)
    L = C.CDLL(REF_LIB)
    f = {k: getattr(L, v) for k, v in SYM.items()}
    for fn in f.values():
        fn.restype = None
    f["ctor"].argtypes = [C.c_void_p]
    f["update"].argtypes = [C.c_void_p, C.c_void_p]
    f["seeds"].argtypes = [C.c_void_p, C.c_int, C.c_int]
    f["line"].argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    f["color"].argtypes = [C.c_void_p, C.c_int]
    f["seed"].argtypes = [C.c_void_p, C.c_uint32]
    f["depth"].argtypes = [C.c_void_p, C.c_int]
    obj = (C.c_uint64 * 8192)()                 # 64 KiB for a FilmGrain (about 10.8 KiB), 8-byte aligned; never destroyed
    fg = C.addressof(obj)
    f["ctor"](fg)
    impl = C.c_uint64.from_address(fg).value
    u8 = lambda off, n: np.frombuffer(C.string_at(impl + off, n), np.uint8)
    # the layout read off the object: the defaults of the constructors, then set_depth moves bs and scale_shift as FilmGrainImpl.cpp:364-374 says
    assert [C.c_uint32.from_address(fg + FG_LINE_RND + 4 * k).value for k in range(3)] == [0xdeadbeef] * 3, "FilmGrain layout"
    assert u8(IMPL_SHIFT, 2).tolist() == [11, 0] and C.c_int.from_address(impl + IMPL_CSUBX).value == 2, "FilmGrainImpl layout"
    f["depth"](impl, 10)
    assert u8(IMPL_SHIFT, 2).tolist() == [9, 2], "FilmGrainImpl layout (set_depth)"
    f["depth"](impl, 8)
    out = {}
    for n, op in enumerate(ops):
        if op[0] == "fgc":
            sei = op[1]
            s = sei_struct(sei)
            f["update"](fg, C.addressof(s))
            fgs = np.frombuffer(C.string_at(fg + FG_FGS, 5), np.uint8)
            assert fgs[0] == sei["model_id"] and fgs[1] == sei["log2_scale_factor"], "FilmGrain layout (fgs)"
            bs = int(u8(IMPL_BS, 1)[0])
            shift = int(u8(IMPL_SHIFT, 1)[0]) - 6 + bs
            assert shift == sei["log2_scale_factor"] - (1 if sei["model_id"] else 0), "scale_shift"
            plut = u8(IMPL_PLUT, 768).reshape(3, 256)
            assert not (plut & 15).any() and (plut < 0x80).all(), "pLUT"
            out["o%d_present" % n] = fgs[2:5].copy()
            out["o%d_shift" % n] = np.array(shift)
            out["o%d_slut" % n] = u8(IMPL_SLUT, 768).reshape(3, 256).copy()
            out["o%d_plut" % n] = plut.copy()
            out["o%d_pattern" % n] = np.frombuffer(C.string_at(impl + IMPL_PATTERN, 2 * 9 * 4096), np.int8).reshape(2, 9, 64, 64)[:, :8].copy()
        elif op[0] == "seed":
            f["seed"](fg, op[1] & 0xffffffff)
        else:
            _, fi, bd, cf = op
            planes = [frames["f%d_c%d" % (fi, k)] for k in range(3 if cf else 1)]
            H, W = planes[0].shape
            dt = np.uint8 if bd == 8 else np.uint16
            # rows padded by 64 samples repeating the last one (the last block of a row writes up to 15 samples past the row's end)
            bufs = [np.ascontiguousarray(np.pad(p.astype(dt), ((0, 0), (0, 64)), mode="edge")) for p in planes]
            f["depth"](impl, bd)
            if cf:
                f["color"](fg, 1)
            f["seeds"](fg, W, H)
            for y in range(H):
                Y = bufs[0].ctypes.data + bufs[0].strides[0] * y
                U = V = None
                if cf:
                    U = bufs[1].ctypes.data + bufs[1].strides[0] * (y // 2)
                    V = bufs[2].ctypes.data + bufs[2].strides[0] * (y // 2)
                f["line"](fg, Y, U, V, y, W)
            for k, b in enumerate(bufs):
                out["o%d_c%d" % (n, k)] = b[:, :planes[k].shape[1]].astype(np.uint16)
    np.savez(nout, **out)


if __name__ == "__main__":
    _main(sys.argv[1], sys.argv[2], sys.argv[3])
