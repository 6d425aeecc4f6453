"""developer helper: the host stage of the IRAP of the benchmark's stream on this machine - one generated 4K I picture of bench.py's mix through vvr_submit
against the stand-in runtime of tests/hoststub (no GPU involved), 8 worker threads, several times.  Prints the wall time of submit .. wait and, from the
VVR_PHASES line of the developer build (vvr_host_build: an I picture built in bands), the host stage itself and its tail: from the moment the last band
is through phase 1 until the picture is built.

Usage: python tools/host_i_picture_stage.py [--threads 8] [--runs 40] [--root DIR]      (--root: the sources of another checkout, e.g. the parent commit's)"""
import argparse, ctypes as C, os, re, statistics, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from vvdec_amd import abi, synth, stream
import bench
import test_host_glue as T

ap = argparse.ArgumentParser()
ap.add_argument("--threads", type=int, default=8)
ap.add_argument("--runs", type=int, default=40)
ap.add_argument("--root", default=ROOT, help="checkout whose tests/hoststub/vvr_host_stub.cpp (and the product sources it includes) is compiled")
a = ap.parse_args()

tmp = tempfile.mkdtemp(prefix="vvr_i_stage_")
lib, log = os.path.join(tmp, "hoststub_o3.so"), os.path.join(tmp, "stderr.txt")
# (-O3 like the product; VVT_NO_LF_STANDIN: the stand-in of k_lf_init is device work, not host stage)
subprocess.check_call(["g++", "-std=c++17", "-O3", "-fPIC", "-shared", "-pthread", "-Wl,-Bsymbolic", "-I" + T.HIP_INC, "-D__HIP_PLATFORM_AMD__", "-DVVR_DEV_ENV", "-DVVT_NO_LF_STANDIN", "-w",
                       os.path.join(a.root, "tests", "hoststub", "vvr_host_stub.cpp"), "-o", lib])
os.environ["VVR_PHASES"] = "1"
L = abi.bind(C.CDLL(lib))
W, H, mix, _, _ = bench.CONFIGS["4k"]
plans, nslots = stream.ra_plan(1, gop=1, seed_poc0_is_external=False)
d = synth.picture_for_plan(plans[0], W, H, seed=1234, tool_flags=bench._tools(abi), **mix)
assert plans[0].slice_type == abi.SLICE_I and len(d.cu) >= 512
p = d.c()
cfg = abi.Config(); cfg.abi_version = abi.VVR_ABI_VERSION; cfg.max_width = W; cfg.max_height = H; cfg.chroma_format = 1; cfg.bit_depth = 10; cfg.log2_ctu = 7
cfg.num_slots = 4; cfg.num_streams = 2; cfg.host_threads = a.threads
ctx = C.c_void_p(); assert L.vvr_create(C.byref(cfg), C.byref(ctx)) == 0
# the library's developer prints go to the C stderr: into a file while the pictures run
sys.stderr.flush()
saved = os.dup(2); fd = os.open(log, os.O_WRONLY | os.O_CREAT | os.O_TRUNC); os.dup2(fd, 2)
wall = []
try:
    for run in range(a.runs + 5):
        t0 = time.perf_counter()
        j = L.vvr_submit(ctx, C.byref(p))
        assert j >= 0 and L.vvr_wait(ctx, j) == 0
        wall.append((time.perf_counter() - t0) * 1e3)
finally:
    os.dup2(saved, 2); os.close(fd)
L.vvr_destroy(ctx)
wall = wall[5:]                      # (the first pictures grow the scratch buffers)
print("4K I picture, %d CUs, %d worker threads, %d runs (ms: median, min .. max)" % (len(d.cu), a.threads, a.runs))
show = lambda name, v: print("  %-46s %.3f   %.3f .. %.3f" % (name, statistics.median(v), min(v), max(v)))
show("submit .. wait (wall)", wall)
rows = [[float(x) for x in re.findall(r"(-?\d+\.\d+)", ln)] for ln in open(log) if "I picture in bands" in ln][5:]
if rows:
    names = ("phase 1", "join", "phase 2 and units", "layout", "last band through phase 1 -> built", "host stage (work lists .. layout)")
    for k, name in enumerate(names):
        show(name, [r[k] for r in rows])
else:
    print("  (no VVR_PHASES line: this checkout does not build I pictures in two phases)")
