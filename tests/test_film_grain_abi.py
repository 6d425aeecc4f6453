"""The film grain bank at the C-ABI boundary without a GPU: vvr_film_grain_bank as a C compiler lays it out in include/vvr.h == the ctypes mirror
(vvdec_amd.abi.FilmGrainBank), and abi.film_grain_bank fills every field from arrays."""
import ctypes as C
import os
import subprocess

import numpy as np

from vvdec_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bank_layout_matches_a_c_compiler(tmp_path):
    cls = abi.FilmGrainBank
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "vvr.h"', 'int main(void){',
             'printf("sizeof %zu\\n", sizeof(vvr_film_grain_bank));']
    want = {"sizeof": C.sizeof(cls)}
    for f in cls._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(vvr_film_grain_bank, %s));' % (f[0], f[0]))
        want[f[0]] = getattr(cls, f[0]).offset
    lines.append("return 0;}")
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict((k, int(v)) for k, v in (l.split() for l in subprocess.check_output([str(exe)]).decode().splitlines()))
    assert got == want
    assert want["sizeof"] == 4 + 3 + 1 + 768 + 768 + 2 * 8 * 64 * 64


def test_bank_from_arrays():
    rng = np.random.default_rng(3)
    f = dict(comp_present=np.array([1, 0, 1]), shift=5, scale_lut=rng.integers(0, 256, (3, 256)), pattern_lut=rng.integers(0, 8, (3, 256)) << 4,
             pattern=rng.integers(-128, 128, (2, 8, 64, 64)))
    b = abi.film_grain_bank(**f)
    assert b.struct_size == C.sizeof(abi.FilmGrainBank) and b.shift == 5 and list(b.comp_present) == [1, 0, 1]
    raw = np.frombuffer(C.string_at(C.addressof(b), C.sizeof(b)), np.uint8)
    o = abi.FilmGrainBank.pattern.offset
    assert np.array_equal(raw[o:].view(np.int8).reshape(2, 8, 64, 64), f["pattern"])
    o = abi.FilmGrainBank.scale_lut.offset
    assert np.array_equal(raw[o:o + 768].reshape(3, 256), f["scale_lut"])
    o = abi.FilmGrainBank.pattern_lut.offset
    assert np.array_equal(raw[o:o + 768].reshape(3, 256), f["pattern_lut"])
