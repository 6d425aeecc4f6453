"""CPU: tests/itrans_replay.cpp - the record of a transform block (tb_record, vvr_device.h) against the TU / CU records of generated pictures, and the pair indexing
of k_itrans's two passes against the plain triple loop - built with the address and undefined-behaviour sanitizers and run as a program of its own."""
import os
import struct
import subprocess
import ctypes as C
import pytest

from vvdec_amd import abi, synth, stream

HERE = os.path.dirname(os.path.abspath(__file__))
HIP_INC = "/opt/rocm/include"

pytestmark = pytest.mark.skipif(not os.path.exists(os.path.join(HIP_INC, "hip", "hip_runtime_api.h")), reason="HIP headers not installed")

TOOLS = (abi.TOOL_SAO_LUMA | abi.TOOL_SAO_CHROMA | abi.TOOL_ALF | abi.TOOL_DEP_QUANT | abi.TOOL_MTS | abi.TOOL_LFNST | abi.TOOL_BDOF | abi.TOOL_DMVR | abi.TOOL_IMPLICIT_MTS)
MIXES = [
    dict(p_intra=0.5, p_lfnst=0.7, p_mip=0.3, p_isp=0.3, p_coded=0.9, p_coded_chroma=0.8, p_jccr=0.3, p_bdpcm=0.2, p_ts=0.2, p_mts=0.4, p_sbt=0.3),
    dict(p_intra=0.6, dual_tree=3.0, p_isp=0.6, p_lfnst=0.6, p_cclm=0.4, p_coded=0.9, p_coded_chroma=0.8, p_split_scale=1.8, log2_ctu=6),
    dict(p_intra=0.4, min_cu_log2=2, p_split_scale=2.0, p_lfnst=0.5, p_mip=0.3, p_cclm=0.4, p_coded=0.9, p_coded_chroma=0.8, p_bdpcm=0.3, log2_ctu=5),
    dict(p_intra=0.5, p_split_scale=0.5, p_lfnst=0.8, p_mip=0.4, p_coded=0.95, p_coded_chroma=0.9),
]


def test_record_and_packed_passes_replayed_on_the_cpu(tmp_path):
    dumps = []
    for k, mix in enumerate(MIXES):
        plans, _ = stream.ra_plan(3, gop=2, seed_poc0_is_external=False)
        for pl in plans:
            d = synth.picture_for_plan(pl, 256, 128, seed=950 + k, tool_flags=TOOLS, **mix)
            assert d.cu.dtype.itemsize == C.sizeof(abi.Cu) and d.tu.dtype.itemsize == C.sizeof(abi.Tu)
            path = str(tmp_path / ("pic_%d_%d.bin" % (k, pl.poc)))
            with open(path, "wb") as f:
                f.write(struct.pack("<4I", d.cu.dtype.itemsize, d.tu.dtype.itemsize, len(d.cu), len(d.tu)))
                f.write(d.cu.tobytes())
                f.write(d.tu.tobytes())
            dumps.append(path)
    exe = str(tmp_path / "itrans_replay")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-strict-aliasing", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-w",
                           "-I" + HIP_INC, "-D__HIP_PLATFORM_AMD__", os.path.join(HERE, "itrans_replay.cpp"), "-o", exe])
    out = subprocess.run([exe] + dumps, capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))      # (addresses and undefined behaviour; the leak check at exit needs ptrace)
    assert out.returncode == 0 and "all equal" in out.stdout, (out.stdout[-2000:], out.stderr[-2000:])
    records = int(out.stdout.split(" records")[0].split()[-1])
    assert records > 2000, out.stdout
