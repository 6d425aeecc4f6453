"""The cases of the mode-table tests: every index of a mode table on every block shape it is legal on.

The third table beside limits_cases.py (ends of the value ranges) and partition_cases.py (ends of the picture partitioning), with the same two users:
tests/test_oracle_vs_ref_modes.py pins every picture on the CPU (oracle against the reference classes), tests/test_gpu_modes.py then runs the same pictures
through the back-end against the oracle.  Nothing here touches a GPU or the reference build.

A case is one family at one block shape (or a small group of shapes) over a few pictures.  A picture is generated with the uniform CU grid of the generator
(Params.grid_w / grid_h) and then REWRITTEN: a `post` step walks the CUs of the subject kind in order and gives each the next entry of the shape's list,
round-robin, with a start taken from the seed - the way rewrite_qp, alf_to_limits and _saturate rewrite records.  What a rewrite keeps consistent is written
at the rewrite (tools/synth.cpp, addCu, is the model).

The LEGAL SET of a case is written down here as rules that cite the reference's condition; it is never read off what the generator drew.  `census` counts,
per entry of the legal set, the instances the pictures hold and the COUNTING instances: CUs with the above and the left neighbour inside the picture (the
reference samples of the first row and column are the flat default: most modes predict the same block from them) whose own samples change when the subject
field is moved to the adjacent entry of the same table - one oracle run per checked instance, until an entry has WANTED of them (intra CUs read their
neighbours); where the subjects read reference pictures only (GPM, plain motion compensation) the moves of all CUs of a picture share their oracle runs and
every instance is checked.  Every entry needs one counting instance; entries that cannot be made are listed by name in IMPOSSIBLE with the reference line
that forbids them.

Families: intra_angular, intra_chroma, intra_mip, intra_isp, lfnst_sets, transform_types, gpm_splits, mc_phases ("Mode coverage")."""
import numpy as np

import refdrv
import limits_cases as lc
from vvdec_amd import abi, synth
from test_gpu_parity import TOOLS_I, TOOLS_A

B, I = abi.SLICE_B, abi.SLICE_I
SIDES = (4, 8, 16, 32, 64)
SHAPES = [(w, h) for w in SIDES for h in SIDES]          # every luma CU shape of an intra CU: maximum transform size 64, minimum 4 (CU sides are powers of two)
WANTED = 2                                               # counting instances per entry the check looks for (at different positions); one is required

# entries of a legal set that cannot be made, by name, with the line that forbids them.  tests/test_oracle_vs_ref_modes.py asserts that the list is no
# longer than it is now
IMPOSSIBLE = {}


class Case:
    """specs: one (W, H, log2_ctu, seed) per picture.  build(case, spec, state) -> (description, reference pictures): `state` is a dict the pictures of one
    case share (the positions of the round-robin lists).  legal: the set of entries.  instances(d) -> [(CU index, [entries])] of the subject CUs;
    move(d, k) -> [undo, ...]: the subject field of CU k moved to the adjacent entry, once per table the CU stands for.
    found: what census counted, for the record"""

    def __init__(self, id, family, specs, build, legal, instances, move, bd=10, cf=1, luma_only=False, also=None, together=False):
        self.id, self.family, self.specs, self.build, self.legal, self.instances, self.move, self.bd, self.cf = id, family, specs, build, legal, instances, move, bd, cf
        # luma_only: the subject is a luma field (the chroma of the CU may follow it or not); also(case, pics, tally): further assertions; together: the CUs of a
        # picture do not read each other, so the moves of all instances share their oracle runs (_census_together)
        self.luma_only, self.also, self.together, self.found = luma_only, also, together, {}
        # own(planes, cu, chroma): the samples an instance is judged by; exempt(entry): the entry counts without both neighbours inside (intra_chroma says which)
        self.own, self.exempt = _own_samples, lambda e: False

    def pictures(self):
        state = {}
        return [self.build(self, spec, state) + (spec[2],) for spec in self.specs]


CASES = []


def _rect(cu):
    return int(cu["x"]), int(cu["y"]), int(cu["w"]), int(cu["h"])


def _inside(cu):
    """both neighbours the prediction reads lie in the picture"""
    return int(cu["x"]) > 0 and int(cu["y"]) > 0


def _own_samples(planes, cu, chroma):
    x, y, w, h = _rect(cu)
    out = [planes[0][y:y + h, x:x + w]]
    if chroma and int(cu["tree"]) != abi.TREE_LUMA:
        out += [planes[c][y >> 1:(y + h) >> 1, x >> 1:(x + w) >> 1] for c in (1, 2)]
    return out


def _census_together(case, n, d, refs, inst, tally):
    """pictures whose CUs do not read each other (inter prediction only, every filter off): the j-th move of every instance in one oracle run; a CU whose own
    samples stay as they are under one of its moves does not count"""
    ks = np.array([k for k, _ in inst])
    assert (d.cu["pred_mode"][ks] == abi.PRED_INTER).all() and not (d.cu["flags"][ks] & abi.CU_CIIP).any(), case.id       # (the subjects read reference pictures only)
    assert int(d.hdr.tool_flags) & abi.TOOL_DEBLOCK_OFF and not int(d.hdr.tool_flags) & lc.FILTERS, case.id
    chroma = case.cf and not case.luma_only
    base = refdrv.oracle_reconstruct(d, refs, flags=refdrv.STOP_AFTER_RECO)
    moves = {k: case.move(d, k) for k, _ in inst}
    bites = {k: True for k, _ in inst}
    for j in range(max([len(m) for m in moves.values()] + [0])):
        undos = [(k, m[j]()) for k, m in moves.items() if j < len(m)]
        try:
            other = refdrv.oracle_reconstruct(d, refs, flags=refdrv.STOP_AFTER_RECO)
        finally:
            for k, undo in reversed(undos):
                undo()
        for k, _ in undos:
            bites[k] &= lc.differ(_own_samples(base, d.cu[k], chroma), _own_samples(other, d.cu[k], chroma))
    assert not lc.differ(base, refdrv.oracle_reconstruct(d, refs, flags=refdrv.STOP_AFTER_RECO)), "%s: a move was not undone" % case.id
    for k, entries in inst:
        if bites[k]:
            for e in entries:
                tally[e][1].add((n, int(d.cu["x"][k]), int(d.cu["y"][k])))


def census(case, pics):
    """-> {entry: [instances, counting instances]}; asserts nothing"""
    tally = {e: [0, set()] for e in case.legal}
    for n, (d, refs, l2) in enumerate(pics):
        base = None
        together = []
        for k, entries in case.instances(d):
            cu = d.cu[k]
            for e in entries:
                assert e in tally, "%s: picture %d holds %r at (%d, %d), which the legal set does not" % (case.id, n, e, int(cu["x"]), int(cu["y"]))
                tally[e][0] += 1
            if case.together:
                if _inside(cu):
                    together.append((k, entries))
                continue
            if not (_inside(cu) or (entries and all(case.exempt(e) for e in entries))) or all(len(tally[e][1]) >= WANTED for e in entries):
                continue
            if base is None:
                base = refdrv.oracle_reconstruct(d, refs, flags=refdrv.STOP_AFTER_RECO)
            own = [a.copy() for a in case.own(base, cu, case.cf and not case.luma_only)]
            bites = True
            for change in case.move(d, k):       # (an MRL CU stands for its mode and for its line: both must matter)
                undo = change()
                try:
                    other = refdrv.oracle_reconstruct(d, refs, flags=refdrv.STOP_AFTER_RECO)
                finally:
                    undo()
                bites &= lc.differ(own, case.own(other, cu, case.cf and not case.luma_only))
            if bites:
                for e in entries:
                    tally[e][1].add((n, int(cu["x"]), int(cu["y"])))
        if together:
            _census_together(case, n, d, refs, together, tally)
    return tally


def present(case, pics):
    """the census against the legal set minus IMPOSSIBLE; the counts go to case.found"""
    tally = census(case, pics)
    missing = sorted((e for e, (n, pos) in tally.items() if not pos and "%s:%r" % (case.family, e) not in IMPOSSIBLE), key=repr)
    case.found = dict(entries=len(tally), instances=sum(n for n, _ in tally.values()), counting=sum(len(pos) for _, pos in tally.values()),
                      entries_with_two=sum(1 for _, pos in tally.values() if len(pos) >= 2), pictures=len(pics))
    if case.also:
        case.also(case, pics, tally)
    assert not missing, "%s: %d of %d entries without a counting instance, e.g. %r (instances of those: %r)" % (case.id, len(missing), len(tally), missing[:6], [tally[e][0] for e in missing[:6]])
    return tally


def held(case, pics):
    """from the records alone: every entry of the legal set (less IMPOSSIBLE) is held by a CU with both neighbours inside the picture, and no CU of the subject
    kind holds an entry outside the set"""
    seen = set()
    for d, refs, l2 in pics:
        for k, entries in case.instances(d):
            assert all(e in case.legal for e in entries), (case.id, entries)
            if _inside(d.cu[k]) or all(case.exempt(e) for e in entries):
                seen.update(entries)
    missing = sorted((e for e in case.legal - seen if "%s:%r" % (case.family, e) not in IMPOSSIBLE), key=repr)
    assert not missing, "%s: %d of %d entries are not in the pictures, e.g. %r" % (case.id, len(missing), len(case.legal), missing[:6])


def _sizes(w, h):
    """picture size of a shape: 256 x 128, or 512 x 256 where that holds fewer than 40 CUs with both neighbours inside"""
    W, H = (256, 128) if (256 // w - 1) * (128 // h - 1) >= 40 else (512, 256)
    return W, H, (W // w - 1) * (H // h - 1)


class _Queue:
    """a list taken round-robin, the position kept in the case's state"""

    def __init__(self, state, key, items, start):
        self.items, self.state, self.key, self.start = items, state, key, start % len(items)
        state.setdefault(key, self.start)

    def next(self):
        v = self.items[self.state[self.key] % len(self.items)]
        self.state[self.key] += 1
        return v


# ----------------------------------------------------------------------------------------------------------------------------------------------------
# intra_angular: luma modes of plain intra CUs (no MIP, ISP, BDPCM), in I pictures (k_intra) and as intra CUs of B pictures (k_intra_leaf)
#
# Legal set, per shape w x h with w, h in 4 .. 64:
#   ("mode", w, h, m), m = 0 .. 66: intra_luma_pred_mode() puts no condition of the block shape on the mode (CABACReader.cpp:1270-1339: MPM index or one of
#     the 61 remaining modes); the wide-angle remap (IntraPrediction.cpp:443, getWideAngle, by the ratio of the sides) and the reference-smoothing threshold (by
#     log2 w + log2 h) are functions of exactly this pair.
#   ("line", w, h, r), r = 1, 2 and ("mode_line", m, r), m = 1 .. 66: extend_ref_line() (CABACReader.cpp:1242-1268) reads multi_ref_idx for every luma CU without
#     BDPCM that does not lie on the first row of a CTU (:1250), MULTI_REF_LINE_IDX = { 0, 1, 2 } in the description's numbering; with a line > 0 the mode is
#     one of the five non-planar MPMs (:1293, :1310-1317) - any of DC and the 65 angular modes for suitable neighbours, never planar.  The two are pairwise:
#     every shape with both lines, every mode with both lines, not the full product - the 132 (mode, line) pairs are dealt out over the 25 shapes
#     (mode_line_share), and a test adds the shares up.
# A rewrite keeps, as addCu does: planar never with a line > 0; no line > 0 on the first row of a CTU; lfnst_intra_mode = the luma mode; a derived chroma mode
# (DM) follows the luma mode; the chroma-tree CU of a local dual tree takes mode, DM and lfnst_intra_mode from the luma CU at its centre (synth.cpp: colMode).
# BDPCM, MIP and ISP CUs are no subjects and stay as drawn.
# ----------------------------------------------------------------------------------------------------------------------------------------------------
MODE_LINE = [(m, r) for m in range(1, 67) for r in (1, 2)]


def mode_line_share(shape):
    """the (mode, line) pairs a shape's case must hold: every 25th of the 132, both lines among them (25 is odd, so the lines alternate)"""
    return [MODE_LINE[j] for j in range(SHAPES.index(shape), len(MODE_LINE), len(SHAPES))]


def _plain_intra(d):
    cu = d.cu
    return np.flatnonzero((cu["pred_mode"] == abi.PRED_INTRA) & ((cu["flags"] & abi.CU_MIP) == 0) & (cu["isp_mode"] == 0) & (cu["bdpcm"][:, 0] == 0) & (cu["tree"] != abi.TREE_CHROMA))


def set_luma_mode(d, k, mode, line=None):
    """-> undo()"""
    cu = d.cu
    keep = (int(cu["intra_dir"][k, 0]), int(cu["intra_dir"][k, 1]), int(cu["lfnst_intra_mode"][k]), int(cu["multi_ref_idx"][k]))
    assert not (mode == 0 and (line if line is not None else keep[3])), "planar with a reference line > 0"
    if int(cu["tree"][k]) != abi.TREE_LUMA and keep[1] == keep[0]:       # the derived chroma mode follows
        cu["intra_dir"][k, 1] = mode
    cu["intra_dir"][k, 0] = cu["lfnst_intra_mode"][k] = mode
    if line is not None:
        cu["multi_ref_idx"][k] = line

    def undo():
        cu["intra_dir"][k, 0], cu["intra_dir"][k, 1], cu["lfnst_intra_mode"][k], cu["multi_ref_idx"][k] = keep
    return undo


def follow_in_chroma_trees(d, before):
    """the chroma-tree CUs of local dual trees after a rewrite of luma modes (`before`: intra_dir[:, 0] as generated): PU::getCoLocatedIntraLumaMode"""
    cu = d.cu
    owner = np.full((d.h4, d.w4), -1, np.int64)
    for k in np.flatnonzero(cu["tree"] != abi.TREE_CHROMA):
        x, y, w, h = _rect(cu[k])
        owner[y >> 2:(y + h) >> 2, x >> 2:(x + w) >> 2] = k
    for k in np.flatnonzero((cu["tree"] == abi.TREE_CHROMA) & (cu["pred_mode"] == abi.PRED_INTRA)):
        x, y, w, h = _rect(cu[k])
        l = owner[(y + h // 2) >> 2, (x + w // 2) >> 2]
        if cu["pred_mode"][l] != abi.PRED_INTRA:
            continue
        old = 0 if cu["flags"][l] & abi.CU_MIP else int(before[l])
        new = 0 if cu["flags"][l] & abi.CU_MIP else int(cu["intra_dir"][l, 0])
        if int(cu["intra_dir"][k, 1]) == old and not cu["bdpcm"][k, 1]:
            cu["intra_dir"][k, 1] = new
        cu["intra_dir"][k, 0] = cu["lfnst_intra_mode"][k] = new


def _angular_post(d, shape, state, seed, lines=True):
    ctu = 1 << int(d.hdr.log2_ctu)
    before = d.cu["intra_dir"][:, 0].copy()
    modes = _Queue(state, "modes", list(range(67)), seed)
    edge = _Queue(state, "edge", list(range(67)), seed * 7)                   # the CUs of the first row and column: they count for nothing, and still vary
    pairs = _Queue(state, "pairs", mode_line_share(shape) if lines else [(1, 1)], seed)
    state.setdefault("eligible", 0)
    for k in _plain_intra(d):
        cu = d.cu[k]
        if (int(cu["w"]), int(cu["h"])) != shape:
            continue
        if not _inside(cu):
            set_luma_mode(d, k, edge.next(), 0)
        elif lines and int(cu["y"]) & (ctu - 1):
            state["eligible"] += 1
            if state["eligible"] % 3 == 0 and state["pairs"] - pairs.start < (WANTED + 1) * len(pairs.items):       # (every pair three times, then modes only)
                set_luma_mode(d, k, *pairs.next())
            else:
                set_luma_mode(d, k, modes.next(), 0)
        else:
            set_luma_mode(d, k, modes.next(), 0)
    follow_in_chroma_trees(d, before)


def _angular_instances(shape):
    def instances(d):
        out = []
        for k in _plain_intra(d):
            cu = d.cu[k]
            s, m, r = (int(cu["w"]), int(cu["h"])), int(cu["intra_dir"][0]), int(cu["multi_ref_idx"])
            if s == shape:
                out.append((k, [("mode",) + s + (m,)] if r == 0 else [("line",) + s + (r,), ("mode_line", m, r)]))
        return out
    return instances


def _angular_move(d, k):
    m, r = int(d.cu["intra_dir"][k, 0]), int(d.cu["multi_ref_idx"][k])
    changes = [lambda: set_luma_mode(d, k, m + 1 if m < 66 else 65)]
    if r:
        changes.append(lambda: set_luma_mode(d, k, m, 3 - r))
    return changes


INTRA_I = dict(p_mip=0.0, p_isp=0.0, p_mrl=0.0, p_bdpcm=0.03, p_cclm=0.2, p_coded=0.6, p_coded_chroma=0.4, p_lfnst=0.3, p_mts=0.2, p_ts=0.05)
INTRA_B = dict(INTRA_I, p_intra=0.75, p_affine=0.1, p_geo=0.1, p_ciip=0.1, p_bi=0.6)


def _angular_case(name, shape, slice_type, seed, l2s=(7, 6), bd=10, cf=1, lines=True, size=None):
    w, h = shape
    W, H, inside = size + ((size[0] // w - 1) * (size[1] // h - 1),) if size else _sizes(w, h)
    share = mode_line_share(shape) if lines else []
    legal = {("mode", w, h, m) for m in range(67)} | ({("line", w, h, r) for r in (1, 2)} | {("mode_line", m, r) for m, r in share} if lines else set())
    # two instances of every mode and three of every pair with a line; in B pictures three CUs of four are intra; a few CUs are BDPCM CUs; some in reserve
    n = int(np.ceil(1.12 * (WANTED * 67 + (WANTED + 1) * len(share)) / (inside * (0.7 if slice_type == B else 0.96))))
    assert n <= 20, "the seeds of the shapes lie 20 apart"
    specs = [(W, H, l2s[i % len(l2s)], seed + i) for i in range(n)]
    tools = TOOLS_I if slice_type == I else TOOLS_A

    def build(case, spec, state):
        W, H, l2, s = spec
        d, refs = lc.one_picture(W, H, l2, s, tools, ("noise", "checker"), slice_type=slice_type, bd=bd, cf=cf, grid_w=w, grid_h=h, min_cu_log2=2 if min(w, h) == 4 else 3,
                                 **(INTRA_I if slice_type == I else INTRA_B))
        _angular_post(d, shape, state, s, lines)
        return d, refs
    CASES.append(Case("intra_angular_%s_%dx%d" % (name, w, h), "intra_angular", specs, build, legal, _angular_instances(shape), _angular_move, bd=bd, cf=cf, luma_only=True))
    CASES[-1].shape = shape


for _k, _s in enumerate(SHAPES):
    _angular_case("i", _s, I, 4000 + 20 * _k)
for _k, _s in enumerate(SHAPES):
    _angular_case("b", _s, B, 4600 + 20 * _k)
# one subset of the shapes again at 8 bit with CTU 32, and one in 4:0:0 (there a 4 x 4 CU is a single-tree CU)
for _k, _s in enumerate([(4, 32), (32, 4), (8, 16), (16, 16), (32, 32)]):
    _angular_case("i_8bit_ctu32", _s, I, 5200 + 20 * _k, l2s=(5,), bd=8, lines=False, size=(256, 128) if _s != (32, 32) else (512, 256))
for _k, _s in enumerate([(4, 4), (8, 4), (16, 8), (64, 16), (32, 64)]):
    _angular_case("i_400", _s, I, 5400 + 20 * _k, cf=0, lines=False)


# ----------------------------------------------------------------------------------------------------------------------------------------------------
# intra_mip: matrix-based intra prediction
#
# Legal set: ("mip", w, h, mode, transposed) for every shape w x h with w, h in 4 .. 64, mode = 0 .. getNumModesMip() - 1, transposed = 0, 1.  mip_flag()
# (CABACReader.cpp:3125-3136) puts no condition on the block shape (the CU fits the maximum transform size of 64); mip_pred_mode() (:3138-3149) reads the
# transposed flag and a truncated-binary mode below getNumModesMip (UnitTools.cpp:3736-3746): 16 for 4 x 4, 8 for a side of 4 or 8 x 8, 6 otherwise
# (getMipSizeId, :3748).  The size class also selects the matrices, the boundary down-sampling and the up-sampling per shape.
# A rewrite keeps: the chroma mode of a MIP CU (planar where it is derived) and lfnst_intra_mode = planar are functions of the flag, not of the mode.
# ----------------------------------------------------------------------------------------------------------------------------------------------------
def mip_modes(w, h):
    return 16 if (w, h) == (4, 4) else 8 if (w == 4 or h == 4 or (w, h) == (8, 8)) else 6


def _mip_cus(d):
    return np.flatnonzero((d.cu["pred_mode"] == abi.PRED_INTRA) & ((d.cu["flags"] & abi.CU_MIP) != 0))


def set_mip_mode(d, k, mode, transposed):
    cu = d.cu
    keep = (int(cu["intra_dir"][k, 0]), int(cu["flags"][k]))
    cu["intra_dir"][k, 0] = mode
    cu["flags"][k] = (keep[1] & ~abi.CU_MIP_TRANSP) | (abi.CU_MIP_TRANSP if transposed else 0)

    def undo():
        cu["intra_dir"][k, 0], cu["flags"][k] = keep
    return undo


def _mip_entry(d, k):
    cu = d.cu[k]
    return ("mip", int(cu["w"]), int(cu["h"]), int(cu["intra_dir"][0]), 1 if int(cu["flags"]) & abi.CU_MIP_TRANSP else 0)


def _mip_instances(shape):
    def instances(d):
        return [(k, [_mip_entry(d, k)]) for k in _mip_cus(d) if (int(d.cu["w"][k]), int(d.cu["h"][k])) == shape]
    return instances


def _mip_move(d, k):
    e = _mip_entry(d, k)
    n = mip_modes(e[1], e[2])
    return [lambda: set_mip_mode(d, k, e[3] + 1 if e[3] + 1 < n else e[3] - 1, e[4])]


MIP = dict(INTRA_I, p_mip=0.8, p_mrl=0.1, p_bdpcm=0.0)


def _mip_case(shape, slice_type, seed):
    w, h = shape
    W, H, inside = _sizes(w, h)
    n_modes = mip_modes(w, h)
    legal = {("mip", w, h, m, t) for m in range(n_modes) for t in (0, 1)}
    n = max(1, int(np.ceil(1.5 * WANTED * 2 * n_modes / (inside * 0.75 * (0.55 if slice_type == B else 1.0)))))
    specs = [(W, H, (7, 6)[i % 2], seed + i) for i in range(n)]
    tools = TOOLS_I if slice_type == I else TOOLS_A

    def build(case, spec, state):
        W, H, l2, s = spec
        d, refs = lc.one_picture(W, H, l2, s, tools, ("noise", "checker"), slice_type=slice_type, grid_w=w, grid_h=h, min_cu_log2=2 if min(w, h) == 4 else 3,
                                 **dict(MIP, **(dict(p_intra=0.6, p_bi=0.6) if slice_type == B else {})))
        q = _Queue(state, "mip", [(m, t) for m in range(n_modes) for t in (0, 1)], s)
        edge = _Queue(state, "edge", [(m, t) for t in (0, 1) for m in range(n_modes)], s * 5)
        for k in _mip_cus(d):
            if (int(d.cu["w"][k]), int(d.cu["h"][k])) == shape:
                set_mip_mode(d, k, *(q.next() if _inside(d.cu[k]) else edge.next()))
        return d, refs
    CASES.append(Case("intra_mip_%s_%dx%d" % ("i" if slice_type == I else "b", w, h), "intra_mip", specs, build, legal, _mip_instances(shape), _mip_move, luma_only=True))
    CASES[-1].shape = shape


for _k, _s in enumerate(SHAPES):
    _mip_case(_s, I if _k % 2 == 0 else B, 5600 + 20 * _k)       # (the shapes alternate between I pictures and intra CUs of B pictures)


# ----------------------------------------------------------------------------------------------------------------------------------------------------
# intra_chroma: chroma modes of single-tree CUs in 4:2:0 (and of the chroma-tree CU of a local dual tree)
#
# A luma CU grid of w x h with w >= 8 holds chroma blocks of w/2 x h/2: 4 .. 32 wide, 2 .. 32 high (a chroma block 2 wide or of fewer than 16 samples does
# not exist: the split that would make one opens a local dual tree, whose chroma CU covers the parent; the grids with w = 4 hold those).
# Legal set, per chroma shape cw x ch:
#   ("chroma", cw, ch, m), m = 0 .. 66: intra_chroma_pred_mode() (CABACReader.cpp:1341-) codes planar, vertical, horizontal, DC, the derived mode - and 66 in
#     place of whichever of the four the derived mode equals.  The derived mode is the luma mode of the CU (4:2:0: as it is), so every m is legal where the luma
#     mode is m too: the rewrite sets both.  The wide-angle remap of a chroma block goes by the chroma block's own sides.
#   ("cclm", cw, ch, m, collocated), m = 67, 68, 69 (LM, MDLM_L, MDLM_T), with sps_chroma_vertical_collocated_flag (VVR_TOOL_CCLM_COLLOC) off and on: CCLM is
#     allowed in every single-tree CU (checkCCLMAllowed restricts dual trees only); the flag selects the luma down-sampling filter.
#   ("cclm_no_above", m, collocated) / ("cclm_no_left", m, collocated): the template of a side that lies outside the picture is missing.  These are the stated
#     exception to the neighbour rule: they count on the first row / column of the picture (and only there; CTU edges at slice and tile boundaries are not built).
# A CU counts if its CHROMA samples change when the chroma mode alone moves to the adjacent one.
# ----------------------------------------------------------------------------------------------------------------------------------------------------
def _chroma_cus(d):
    cu = d.cu
    return np.flatnonzero((cu["pred_mode"] == abi.PRED_INTRA) & (cu["tree"] != abi.TREE_LUMA) & (cu["bdpcm"][:, 1] == 0))


def set_chroma_mode(d, k, mode):
    keep = int(d.cu["intra_dir"][k, 1])
    d.cu["intra_dir"][k, 1] = mode

    def undo():
        d.cu["intra_dir"][k, 1] = keep
    return undo


def missing_templates(d, cu):
    """(above, left): why the neighbour on that side is not available to the CU - "picture": it lies outside; "tile" / "slice": it lies in another tile / slice
    (a CU on the first row / column of a CTU there; availability goes by tile and slice membership, CodingStructure::getCURestricted) - or None"""
    l2 = int(d.hdr.log2_ctu)
    cx = (int(d.hdr.width) + (1 << l2) - 1) >> l2
    x, y = int(cu["x"]), int(cu["y"])
    out = []
    for nx, ny in ((x, y - 1), (x - 1, y)):
        if nx < 0 or ny < 0:
            out.append("picture")
            continue
        a, b = (y >> l2) * cx + (x >> l2), (ny >> l2) * cx + (nx >> l2)
        if d.ctu_tile is not None and d.ctu_tile[a] != d.ctu_tile[b]:
            out.append("tile")
        elif d.ctu_slice is not None and d.ctu_slice[a] != d.ctu_slice[b]:
            out.append("slice")
        else:
            out.append(None)
    return tuple(out)


def _chroma_instances(cshape, collocated, dual):
    def instances(d):
        out = []
        for k in _chroma_cus(d):
            cu = d.cu[k]
            m, s = int(cu["intra_dir"][1]), (int(cu["w"]) >> 1, int(cu["h"]) >> 1)
            if s != cshape:
                continue
            gone = missing_templates(d, cu)
            if m < 67:
                out.append((k, [("chroma_dual" if dual else "chroma",) + s + (m,)]))
            elif gone == (None, None):
                out.append((k, [("cclm_dual" if dual else "cclm",) + s + (m, collocated)]))
            else:
                out.append((k, [(name, m, collocated, why) for name, why in zip(("cclm_no_above", "cclm_no_left"), gone) if why]))
        return out
    return instances


def _cclm_templates(d, m, cu):
    """(above, left): the templates a CCLM mode reads at this position"""
    gone = missing_templates(d, cu)
    return (m in (67, 69) and not gone[0], m in (67, 68) and not gone[1])


def _chroma_move(d, k):
    """the adjacent mode; for CCLM the next of the three that reads other templates here (on the first row LM and MDLM_L both read the left one alone)"""
    cu, m = d.cu[k], int(d.cu["intra_dir"][k, 1])
    if m < 67:
        return [lambda: set_chroma_mode(d, k, m + 1 if m < 66 else 65)]
    others = [x for x in (68, 69, 67, 68) if x != m]
    to = ([x for x in others if _cclm_templates(d, x, cu) != _cclm_templates(d, m, cu)] + others)[0]
    return [lambda: set_chroma_mode(d, k, to)]


def _own_chroma(planes, cu, chroma):
    x, y, w, h = _rect(cu)
    return [planes[c][y >> 1:(y + h) >> 1, x >> 1:(x + w) >> 1] for c in (1, 2)]


CHROMA = dict(INTRA_I, p_cclm=0.0, p_bdpcm=0.0, p_coded_chroma=0.5)


def _chroma_case(shape, seed, collocated, dual=False, parts=None):
    """dual: an I picture with separate trees (dual_tree = 1: chroma-tree CUs on the grid, at least 8 x 8 luma samples); parts: "tiles" - 2 x 2 tiles - or "slices" -
    two bands of CTU rows -, a case about the CCLM CUs beside those boundaries alone"""
    w, h = shape
    pw, ph = (8, max(h, 8)) if w == 4 else (w, h)       # (w = 4: the chroma-tree CU of the local dual tree covers the parent of two or four luma CUs)
    cw, ch = pw >> 1, ph >> 1
    W, H, inside = _sizes(pw, ph)
    if parts:
        legal = {(nm, m, collocated, "tile") for nm in ("cclm_no_above", "cclm_no_left") for m in (67, 68, 69)} if parts == "tiles" else {("cclm_no_above", m, collocated, "slice") for m in (67, 68, 69)}
        n, cclm = 2, True
    else:
        # dual trees: no CCLM where the 64 x 64 luma node is split in two first (checkCCLMAllowed, UnitTools.cpp:3476-3483) - the grids with one side of 64
        cclm = not (dual and max(w, h) == 64 and (w, h) != (64, 64))
        legal = {("chroma_dual" if dual else "chroma", cw, ch, m) for m in range(67)}
        if cclm:
            legal |= {("cclm_dual" if dual else "cclm", cw, ch, m, collocated) for m in (67, 68, 69)} | {(nm, m, collocated, "picture") for nm in ("cclm_no_above", "cclm_no_left") for m in (67, 68, 69)}
        n = max(int(np.ceil(1.15 * WANTED * 70 / inside)), 3 if min(H // ph, W // pw) <= 4 else 1)       # (a first column of four CUs, one of them in the corner and the next below a flat one: three pictures)
    specs = [(W, H, 6 if parts else (7, 6)[i % 2], seed + i) for i in range(n)]
    tools = TOOLS_I | (abi.TOOL_CCLM_COLLOC if collocated else 0)
    kw = dict(CHROMA, **(dict(dual_tree=1.0) if dual else {}))
    kw.update(dict(tile_cols=2, tile_rows=2) if parts == "tiles" else dict(num_slices=2) if parts == "slices" else {})

    def build(case, spec, state):
        W, H, l2, s = spec
        d, refs = lc.one_picture(W, H, l2, s, tools, (), slice_type=I, grid_w=w, grid_h=h, min_cu_log2=2 if min(w, h) == 4 else 3, **kw)
        q = _Queue(state, "modes", list(range(70)) if not parts else [67, 68, 69], s)
        edge = _Queue(state, "edge", [67, 68, 69, 5, 67, 68, 69, 40], s)
        before = d.cu["intra_dir"][:, 0].copy()
        c = d.cu
        for k in _chroma_cus(d):
            cu = c[k]
            m = q.next() if missing_templates(d, cu) == (None, None) or parts else edge.next()
            if m >= 67 and not cclm:
                m -= 27                               # (no CCLM in this tree)
            if m < 67 and int(cu["tree"]) == abi.TREE_JOINT and not (cu["flags"] & abi.CU_MIP) and not cu["isp_mode"] and not cu["bdpcm"][0]:
                set_luma_mode(d, k, m, 0)             # the derived mode: luma and chroma hold m
            elif m < 67 and int(cu["tree"]) == abi.TREE_CHROMA:       # (local) dual tree: the luma CUs under the chroma CU hold m (the one at its centre decides)
                x, y, pw_, ph_ = _rect(cu)
                for l in np.flatnonzero((c["tree"] == abi.TREE_LUMA) & (c["x"] >= x) & (c["x"] < x + pw_) & (c["y"] >= y) & (c["y"] < y + ph_) & ((c["flags"] & abi.CU_MIP) == 0) & (c["bdpcm"][:, 0] == 0)):
                    set_luma_mode(d, l, m, 0)
            set_chroma_mode(d, k, m)
        follow_in_chroma_trees(d, before)
        return d, refs
    name = "intra_chroma_%s%s%dx%d" % ("dual_tree_" if dual else "", "collocated_" if collocated else "", cw, ch) + ("_chroma_tree" if w == 4 else "") + ("_" + parts if parts else "")
    c = Case(name, "intra_chroma", specs, build, legal, _chroma_instances((cw, ch), collocated, dual), _chroma_move)
    c.own, c.exempt, c.shape = _own_chroma, lambda e: e[0].startswith("cclm_no_"), shape
    if parts:       # (the other CUs of these pictures are no subjects)
        inner = c.instances
        c.instances = lambda d: [(k, [e for e in es if e in legal]) for k, es in inner(d) if any(e in legal for e in es)]
    CASES.append(c)


# (no luma grid of 8 x 4: a chroma block of 4 x 2 has fewer than 16 samples, the split that would make one opens a local dual tree - the 4 x 4 chroma-tree case)
CHROMA_GRIDS = [(w, h) for w in SIDES[1:] for h in SIDES if (w, h) != (8, 4)] + [(4, 4), (4, 16), (4, 64)]
for _k, _s in enumerate(CHROMA_GRIDS):       # the flag alternates over the shapes ...
    _chroma_case(_s, 7600 + 20 * _k, _k & 1)
for _k, _s in enumerate([(8, 8), (16, 4), (16, 32), (64, 64), (64, 4), (4, 16)]):       # ... and one subset has the other value too
    _chroma_case(_s, 8100 + 20 * _k, 1 - (CHROMA_GRIDS.index(_s) & 1))
# the chroma trees of dual-tree I pictures: chroma-tree CUs of 8 .. 64 x 8 .. 64 luma samples, 4 .. 32 x 4 .. 32 chroma samples
for _k, _s in enumerate([(w, h) for w in SIDES[1:] for h in SIDES[1:]]):
    _chroma_case(_s, 8300 + 20 * _k, (_k + 1) & 1, dual=True)
# CCLM beside tile and slice boundaries inside the picture, both settings of the flag
for _k, (_s, _p) in enumerate([((8, 8), "tiles"), ((16, 16), "tiles"), ((32, 8), "tiles"), ((8, 8), "slices"), ((16, 32), "slices"), ((8, 16), "tiles")]):
    _chroma_case(_s, 8700 + 20 * _k, _k & 1, parts=_p)
_chroma_case((16, 16), 8900, 1, dual=True, parts="tiles")


# ----------------------------------------------------------------------------------------------------------------------------------------------------
# intra_isp: intra sub-partitions
#
# Legal set: ("isp", w, h, direction, lfnst_idx > 0).  isp_mode() (CABACReader.cpp:2541-2580) reads a direction - 1 horizontal, 2 vertical - for every luma CU
# without a reference line > 0 and without BDPCM for which canUseISPSplit (UnitTools.cpp:343-358) allows it: more than 16 samples and no side above the maximum
# transform size of 64; both directions or none.  So every shape but 4 x 4: 4 x 8 and 8 x 4 in two partitions, the others in four (getISPSplitDim, :360), down to
# partitions one and two samples wide or high on the shapes with a side of 4.  lfnst_idx > 0 only where the partitions are at least 4 x 4
# (canUseLfnstWithISP, :319-335).
# The direction decides the transform units, so it is drawn, not rewritten (p_isp; both directions come up by themselves); the luma modes of the ISP CUs are
# rewritten in turn like those of the plain CUs, and a CU counts if its samples change with its mode.
# ----------------------------------------------------------------------------------------------------------------------------------------------------
def isp_parts(w, h):
    return 2 if (w, h) in ((4, 8), (8, 4)) else 4


def isp_lfnst_allowed(w, h, direction):
    n = isp_parts(w, h)
    pw, ph = (w, h // n) if direction == 1 else (w // n, h)
    return pw >= 4 and ph >= 4


def _isp_cus(d):
    return np.flatnonzero((d.cu["pred_mode"] == abi.PRED_INTRA) & (d.cu["isp_mode"] != 0))


def _isp_instances(shape):
    def instances(d):
        return [(k, [("isp",) + shape + (int(d.cu["isp_mode"][k]), 1 if d.cu["lfnst_idx"][k] else 0)]) for k in _isp_cus(d) if (int(d.cu["w"][k]), int(d.cu["h"][k])) == shape]
    return instances


ISP = dict(INTRA_I, p_isp=0.85, p_bdpcm=0.0, p_lfnst=0.5, p_coded=0.8)


def _isp_case(shape, seed):
    w, h = shape
    W, H, inside = _sizes(w, h)
    legal = {("isp", w, h, dr, f) for dr in (1, 2) for f in (0, 1) if f == 0 or isp_lfnst_allowed(w, h, dr)}
    specs = [(W, H, (7, 6)[i % 2], seed + i) for i in range(1 if inside >= 40 else 3)]

    def build(case, spec, state):
        W, H, l2, s = spec
        d, refs = lc.one_picture(W, H, l2, s, TOOLS_I, (), slice_type=I, grid_w=w, grid_h=h, min_cu_log2=2 if min(w, h) == 4 else 3, **ISP)
        before = d.cu["intra_dir"][:, 0].copy()
        q = _Queue(state, "modes", list(range(67)), s)
        for k in _isp_cus(d):
            set_luma_mode(d, k, q.next())
        follow_in_chroma_trees(d, before)
        return d, refs
    CASES.append(Case("intra_isp_%dx%d" % (w, h), "intra_isp", specs, build, legal, _isp_instances(shape), _angular_move, luma_only=True))
    CASES[-1].shape = shape


for _k, _s in enumerate(SHAPES[1:]):
    _isp_case(_s, 6800 + 5 * _k)


# ----------------------------------------------------------------------------------------------------------------------------------------------------
# gpm_splits: the 64 split directions of the geometric partitioning mode
#
# Legal set: ("gpm", w, h, split), split = 0 .. 63 (merge_gpm_partition_idx, GEO_NUM_PARTITION_MODE = 64, CommonDef.h:369), on every shape with geoAvailable
# (CABACReader.cpp:1752-1755): a B slice, both sides in GEO_MIN_CU_SIZE .. GEO_MAX_CU_SIZE = 8 .. 64 (CommonDef.h:364-367) and neither side 8 times the other or
# more - 14 shapes: all of 8 .. 64 but 8 x 64 and 64 x 8.  Angle and distance index of a split, the mirroring of the weight mask and its offset per shape
# (Rom.cpp:540-570) are functions of exactly this pair.
# Prediction only (limits_cases.no_filters): a rewrite of geo_split_dir leaves the stored motion and the edge tables as drawn, and those are read by filters only.
# ----------------------------------------------------------------------------------------------------------------------------------------------------
GPM_SHAPES = [(w, h) for w in SIDES[1:] for h in SIDES[1:] if w < 8 * h and h < 8 * w]
GPM = dict(p_coded=0.0, p_coded_chroma=0.0, p_intra=0.0, p_geo=0.85, p_bi=0.6, p_affine=0.0)


def _gpm_cus(d):
    return np.flatnonzero((d.cu["pred_mode"] == abi.PRED_INTER) & (d.cu["mc_mode"] == abi.MC_GEO))


def set_split(d, k, split):
    keep = int(d.cu["geo_split_dir"][k])
    d.cu["geo_split_dir"][k] = split

    def undo():
        d.cu["geo_split_dir"][k] = keep
    return undo


def same_list(cu):
    return (int(cu["geo_dir_ref"][0]) >> 4) == (int(cu["geo_dir_ref"][1]) >> 4)


def _gpm_instances(shape):
    def instances(d):
        return [(k, [("gpm", int(d.cu["w"][k]), int(d.cu["h"][k]), int(d.cu["geo_split_dir"][k]))]) for k in _gpm_cus(d) if (int(d.cu["w"][k]), int(d.cu["h"][k])) == shape]
    return instances


def _gpm_also(case, pics, tally):
    """both parts from the same list and from different lists, among the CUs with both neighbours inside"""
    n = [0, 0]
    for d, refs, l2 in pics:
        for k, _ in case.instances(d):
            if _inside(d.cu[k]):
                n[1 if same_list(d.cu[k]) else 0] += 1
    case.found["parts_from_two_lists"], case.found["parts_from_one_list"] = n
    assert n[0] > 0 and n[1] > 0, n


def _gpm_move(d, k):
    s = int(d.cu["geo_split_dir"][k])
    return [lambda: set_split(d, k, s + 1 if s < 63 else 62)]


def _gpm_case(name, shape, seed, cf=1, kinds=("noise", "checker")):
    w, h = shape
    W, H, inside = _sizes(w, h)
    legal = {("gpm", w, h, s) for s in range(64)}
    n = int(np.ceil(1.3 * WANTED * 64 / (inside * 0.8)))
    specs = [(W, H, (7, 6)[i % 2], seed + i) for i in range(n)]

    def build(case, spec, state):
        W, H, l2, s = spec
        d, refs = lc.one_picture(W, H, l2, s, lc.no_filters(TOOLS_A), kinds, slice_type=B, cf=cf, grid_w=w, grid_h=h, **GPM)
        q = _Queue(state, "gpm", list(range(64)), s)
        edge = _Queue(state, "edge", list(range(64)), s * 3)
        for k in _gpm_cus(d):
            set_split(d, k, q.next() if _inside(d.cu[k]) else edge.next())
        return d, refs
    CASES.append(Case("gpm_splits_%s%dx%d" % (name, w, h), "gpm_splits", specs, build, legal, _gpm_instances(shape), _gpm_move, cf=cf, also=_gpm_also, together=True))
    CASES[-1].shape = shape


for _k, _s in enumerate(GPM_SHAPES):
    _gpm_case("", _s, 6200 + 20 * _k)
for _k, _s in enumerate([(8, 8), (16, 32), (64, 64)]):
    _gpm_case("400_", _s, 6600 + 20 * _k, cf=0)


# ----------------------------------------------------------------------------------------------------------------------------------------------------
# mc_phases: the two interpolation filter banks of plain uni- and bi-predicted CUs
#
# A vector is stored in 1/16 luma sample (MV_FRACTIONAL_BITS_INTERNAL = 4, CommonDef.h:265).  xPredInterBlk takes the filter of a direction by
# mv & ( ( 1 << ( 4 + chroma scale ) ) - 1 ) (InterPrediction.cpp:777-778): 16 luma phases per axis and, in 4:2:0, 32 chroma phases per axis; both axes
# fractional is the separable path (:859-860), one of them the one-pass paths (:830, :834), and the SIMD tiles differ by block width (:846, :850).  With
# imv == IMV_HPEL the luma phase 8 takes the smoothing half-sample filter instead (useAltHpelIf, :775); such a vector is a multiple of 8.
# Legal set of a case (a CU grid of one shape): ("x", width class, px) and ("y", height class, py), 16 phases each, with the classes 4, 8, 16 (and above) the
# tiles treat differently; ("hpel", width class, height class) for imv == 3 at phase 8 in both axes; and in the two cases that carry the pairs - 8 x 8 and
# 16 x 16 CUs - ("luma", px, py) for the 16 x 16 pairs mv & 15 and ("chroma", px, py) for the 32 x 32 pairs mv & 31.  A CU stands for the entries of every
# list it predicts from, and counts if its samples change when either component of either vector moves to the adjacent phase of the same sample position
# (a half-sample CU: when imv is cleared).  The subjects read reference pictures only, so the moves of all CUs of a picture share their oracle runs.
# A rewrite replaces the five low bits of both components (two for the half-sample CUs: multiples of 8 stay multiples of 8) and keeps, as addCu does: the
# CU's vector in the motion field, and mc_mode = uni for a bi-predicted CU whose two lists hold the same picture and the same vector (xCheckIdenticalMotion).
# Prediction only, no BDOF / DMVR / PROF in the tool flags: what k_mc writes is what the picture holds.
# ----------------------------------------------------------------------------------------------------------------------------------------------------
MCP = dict(p_coded=0.0, p_coded_chroma=0.0, p_intra=0.0, p_imv_hpel=0.12, p_bi=0.6, p_bcw=0.0, mv_sigma=6.0)


def _cls(side):
    return min(side, 16)


def _plain_inter(d):
    cu = d.cu
    return np.flatnonzero((cu["pred_mode"] == abi.PRED_INTER) & ((cu["mc_mode"] == abi.MC_UNI) | (cu["mc_mode"] == abi.MC_BI)) & ((cu["flags"] & abi.CU_CIIP) == 0))


def set_vector(d, k, l, mv=None, imv=None):
    """the vector of list l of a plain CU (and / or its imv), consistent in the motion field and in mc_mode -> undo()"""
    cu = d.cu
    keep = (cu["mv"][k].copy(), int(cu["imv"][k]), int(cu["mc_mode"][k]))
    cells = lc.cu_cells(d, cu[k])
    keep_cells = cells["mv"].copy()
    if mv is not None:
        cu["mv"][k, l, 0] = mv
        cells["mv"][:, :, l] = mv
    if imv is not None:
        cu["imv"][k] = imv
    r = cu["ref_idx"][k]
    if r[0] >= 0 and r[1] >= 0:
        same = int(d.hdr.ref_poc[0][int(r[0])]) == int(d.hdr.ref_poc[1][int(r[1])]) and (cu["mv"][k, 0, 0] == cu["mv"][k, 1, 0]).all()
        cu["mc_mode"][k] = abi.MC_UNI if same else abi.MC_BI

    def undo():
        cu["mv"][k], cu["imv"][k], cu["mc_mode"][k] = keep
        cells["mv"][...] = keep_cells
    return undo


def _phase_instances(shape, chroma):
    def instances(d):
        out = []
        for k in _plain_inter(d):
            cu = d.cu[k]
            w, h = int(cu["w"]), int(cu["h"])
            if (w, h) != shape:
                continue
            e = []
            for l in range(2):
                if cu["ref_idx"][l] < 0:
                    continue
                x, y = int(cu["mv"][l, 0, 0]), int(cu["mv"][l, 0, 1])
                if int(cu["imv"]) == 3:       # (the phases 0 and 8 of these CUs take other filters: they are no instances of the regular banks)
                    if (x & 15, y & 15) == (8, 8):
                        e.append(("hpel", _cls(w), _cls(h)))
                    continue
                e += [("x", _cls(w), x & 15), ("y", _cls(h), y & 15)]
                if chroma:
                    e += [("luma", x & 15, y & 15), ("chroma", x & 31, y & 31)]
            if e:
                out.append((k, sorted(set(e))))
        return out
    return instances


def _phase_move(d, k):
    cu = d.cu[k]
    if int(cu["imv"]) == 3:
        return [lambda: set_vector(d, k, 0, imv=0)]
    changes = []
    for l in range(2):
        if cu["ref_idx"][l] >= 0:
            for a in range(2):
                mv = cu["mv"][l, 0].copy()
                mv[a] += 1 if (int(mv[a]) & 31) < 31 else -1       # the adjacent phase of the same sample position
                changes.append(lambda l=l, mv=mv: set_vector(d, k, l, mv=mv))
    return changes


def _phase_case(shape, seed, chroma, size, cf=1):
    w, h = shape
    legal = {("x", _cls(w), x) for x in range(16)} | {("y", _cls(h), y) for y in range(16)} | {("hpel", _cls(w), _cls(h))}
    if chroma:
        legal |= {("luma", x, y) for x in range(16) for y in range(16)} | {("chroma", x, y) for x in range(32) for y in range(32)}
    # the pairs of the 32 x 32 phases in turn; in the cases that are about the block size classes alone, four diagonals of them
    pairs = [(x, y) for x in range(32) for y in range(32)] if chroma else [(x, (x + 9 * j + 5) & 31) for j in range(4) for x in range(32)]
    # vectors per CU with both neighbours inside: a CU of 4 x 8 has one list, the others 1.6 on average; an eighth are half-sample CUs, and every fourth vector
    # of those holds phase 8 in both axes; a third in reserve (twice that for the half-sample CUs, which are drawn)
    inside = (size[0] // w - 1) * (size[1] // h - 1)
    lists = 1.0 if w + h <= 12 else 1.6
    pictures = int(np.ceil(max(1.35 * WANTED * len(pairs) / (inside * 0.88 * lists), 2.0 * WANTED * 4 / (inside * 0.12 * lists))))
    assert pictures <= 20, "the seeds of the shapes lie 20 apart"
    specs = [size + ((7, 6)[i % 2], seed + i) for i in range(pictures)]

    def build(case, spec, state):
        W, H, l2, s = spec
        d, refs = lc.one_picture(W, H, l2, s, lc.no_filters(TOOLS_I), ("noise", "taps") if s & 1 else ("taps", "noise"), slice_type=B, cf=cf, grid_w=w, grid_h=h,
                                 min_cu_log2=2 if min(w, h) == 4 else 3, **MCP)
        q = _Queue(state, "pairs", pairs, s * 37)
        edge = _Queue(state, "edge", pairs, s * 11)
        half = _Queue(state, "half", [(8, 8), (24, 24), (8, 24), (24, 8), (0, 8), (8, 0), (16, 24), (24, 16), (0, 0), (16, 16), (0, 16), (16, 0), (0, 24), (24, 0), (8, 16), (16, 8)], s)
        for k in _plain_inter(d):
            cu = d.cu[k]
            for l in range(2):
                if cu["ref_idx"][l] >= 0:
                    p = half.next() if int(cu["imv"]) == 3 else q.next() if _inside(cu) else edge.next()
                    set_vector(d, k, l, mv=(cu["mv"][l, 0] & ~31) | np.array(p, np.int32))
        return d, refs
    CASES.append(Case("mc_phases_%s%dx%d" % ("" if cf else "400_", w, h), "mc_phases", specs, build, legal, _phase_instances(shape, chroma), _phase_move, cf=cf, together=True))
    CASES[-1].shape = shape


_phase_case((8, 8), 7000, True, (256, 128))
_phase_case((16, 16), 7020, True, (512, 256))
for _k, _s in enumerate([(4, 8), (8, 4), (4, 16), (16, 4), (4, 64), (64, 4), (8, 32), (32, 8), (32, 32), (64, 16), (16, 64), (64, 64)]):
    _phase_case(_s, 7040 + 20 * _k, False, (256, 128) if _s[0] * _s[1] <= 256 else (512, 256))
_phase_case((8, 8), 7400, False, (256, 128), cf=0)
_phase_case((16, 32), 7420, False, (512, 256), cf=0)


# ----------------------------------------------------------------------------------------------------------------------------------------------------
# lfnst_sets: the LFNST kernels
#
# residual_lfnst_mode() (CABACReader.cpp:2570-2620) reads lfnst_idx 1 or 2 for an intra CU whose transform blocks are at least 4 x 4 and at most the maximum
# transform size, without transform skip, MIP below 16 x 16 or ISP partitions below 4 x 4; the kernel is selected by the set of the intra mode - after the
# wide-angle remap by the block's sides - its transposition (modes above 34) and lfnst_idx, and its support by the block class: 4 x 4, 8 x 8, a side of 4 with
# the other of 8 or more, both sides 8 or more with one above 8.
# Legal set of a case (a luma CU grid of one shape): ("lfnst", w, h, lfnst_idx, mode), lfnst_idx = 1, 2, mode = 0 .. 66 - per shape, which holds every class
# (LFNST_SHAPES has several shapes of each, the non-square ones reach the wide angles).  In dual-tree pictures also ("lfnst_chroma", cw, ch, lfnst_idx, mode,
# "cclm"): chroma-tree CUs whose chroma mode is a CCLM mode; their lfnst_intra_mode is the luma mode at the centre (planar under MIP).
# A rewrite gives the luma CUs (mode, lfnst_idx) pairs in turn; lfnst_intra_mode follows the mode (set_luma_mode, follow_in_chroma_trees), the levels stay as
# drawn for an LFNST block.  A CU counts if its samples change when lfnst_intra_mode moves 33 modes on (another set or the other transposition for every mode and every
# wide-angle remap, where 17 on lands on the same kernel for some; for luma CUs the set goes by the luma mode itself, so the prediction moves too) and when lfnst_idx alone moves to the other value.
# ----------------------------------------------------------------------------------------------------------------------------------------------------
LFNST_SHAPES = [(4, 4), (8, 8), (4, 8), (8, 4), (4, 32), (32, 4), (16, 4), (8, 16), (16, 8), (16, 16), (8, 32), (32, 8), (32, 32), (64, 16), (64, 64)]


def lfnst_class(w, h):
    return "4x4" if (w, h) == (4, 4) else "8x8" if (w, h) == (8, 8) else "4xN" if min(w, h) == 4 else "8xN"


def _lfnst_cus(d):
    cu = d.cu
    return np.flatnonzero((cu["pred_mode"] == abi.PRED_INTRA) & (cu["lfnst_idx"] != 0) & ((cu["flags"] & abi.CU_MIP) == 0) & (cu["isp_mode"] == 0))


def set_lfnst(d, k, mode=None, idx=None):
    keep = (int(d.cu["lfnst_intra_mode"][k]), int(d.cu["lfnst_idx"][k]))
    if mode is not None:
        d.cu["lfnst_intra_mode"][k] = mode
    if idx is not None:
        d.cu["lfnst_idx"][k] = idx

    def undo():
        d.cu["lfnst_intra_mode"][k], d.cu["lfnst_idx"][k] = keep
    return undo


def _lfnst_instances(shape):
    def instances(d):
        out = []
        for k in _lfnst_cus(d):
            cu = d.cu[k]
            w, h, t, idx, m = int(cu["w"]), int(cu["h"]), int(cu["tree"]), int(cu["lfnst_idx"]), int(cu["lfnst_intra_mode"])
            if (w, h) != shape:
                continue
            if t != abi.TREE_CHROMA:
                if not int(d.hdr.slice_type) == I or not (d.cu["tree"] == abi.TREE_CHROMA).any() or min(w, h) == 4:       # (the dual-tree cases are about the chroma trees)
                    out.append((k, [("lfnst", w, h, idx, m)]))
            elif int(cu["intra_dir"][1]) >= 67:
                out.append((k, [("lfnst_chroma", w >> 1, h >> 1, idx, m, "cclm")]))
        return out
    return instances


def _lfnst_move(d, k):
    m, idx = int(d.cu["lfnst_intra_mode"][k]), int(d.cu["lfnst_idx"][k])
    if int(d.cu["tree"][k]) != abi.TREE_CHROMA:       # (luma: the set goes by the luma mode itself, lfnst_intra_mode is read for chroma only - so the prediction moves too)
        return [lambda: set_luma_mode(d, k, (m + 33) % 67), lambda: set_lfnst(d, k, idx=3 - idx)]
    return [lambda: set_lfnst(d, k, mode=(m + 33) % 67), lambda: set_lfnst(d, k, idx=3 - idx)]


LFNST = dict(INTRA_I, p_lfnst=0.9, p_bdpcm=0.0, p_coded=0.8, p_cclm=0.4, p_ts=0.0)


def _lfnst_case(shape, seed, dual=False):
    w, h = shape
    W, H, inside = _sizes(w, h)
    pairs = [(m, i) for m in range(67) for i in (1, 2)]
    legal = {("lfnst_chroma", w >> 1, h >> 1, i, m, "cclm") for m, i in pairs} if dual else {("lfnst", w, h, i, m) for m, i in pairs}
    n = int(np.ceil(1.2 * WANTED * len(pairs) * (4.2 if dual else 1) / (inside * 0.85)))
    assert n <= 20, (shape, n)
    specs = [(W, H, (7, 6)[i % 2], seed + i) for i in range(n)]

    def build(case, spec, state):
        W, H, l2, s = spec
        d, refs = lc.one_picture(W, H, l2, s, TOOLS_I, (), slice_type=I, grid_w=w, grid_h=h, min_cu_log2=2 if min(w, h) == 4 else 3, **dict(LFNST, **(dict(dual_tree=1.0, p_cclm=0.85, p_coded_chroma=0.95, p_jccr=0.0) if dual else {})))
        before = d.cu["intra_dir"][:, 0].copy()
        q = _Queue(state, "pairs", pairs, s * 3)
        edge = _Queue(state, "edge", pairs, s * 5)
        c = d.cu
        for k in _lfnst_cus(d):
            if int(c["tree"][k]) == abi.TREE_CHROMA:
                continue
            m, i = q.next() if _inside(c[k]) else edge.next()
            if not c["bdpcm"][k, 0]:
                set_luma_mode(d, k, m, 0 if m == 0 else None)
                c["lfnst_idx"][k] = i
        if dual:       # the luma CUs without LFNST as well: the chroma-tree CUs take their modes, and those shall vary too
            for k in _plain_intra(d):
                if not c["lfnst_idx"][k]:
                    set_luma_mode(d, k, q.next()[0], 0)
            qc = _Queue(state, "chroma", pairs, s * 7)
            for k in np.flatnonzero((c["tree"] == abi.TREE_CHROMA) & (c["lfnst_idx"] != 0) & (c["intra_dir"][:, 1] >= 67)):       # the luma CU at the centre decides
                m, i = qc.next() if _inside(c[k]) else edge.next()
                x, y, pw_, ph_ = _rect(c[k])
                for l in np.flatnonzero((c["tree"] == abi.TREE_LUMA) & (c["x"] <= x + pw_ // 2) & (c["x"] + c["w"] > x + pw_ // 2) & (c["y"] <= y + ph_ // 2) & (c["y"] + c["h"] > y + ph_ // 2)):
                    if not (c["flags"][l] & abi.CU_MIP) and not c["bdpcm"][l, 0] and not c["isp_mode"][l]:
                        set_luma_mode(d, l, m, 0 if m == 0 else None)
                c["lfnst_idx"][k] = i
        follow_in_chroma_trees(d, before)
        return d, refs
    CASES.append(Case("lfnst_sets_%s%dx%d" % ("dual_tree_" if dual else "", w, h), "lfnst_sets", specs, build, legal, _lfnst_instances(shape), _lfnst_move, luma_only=not dual))
    CASES[-1].shape = shape


for _k, _s in enumerate(LFNST_SHAPES):
    _lfnst_case(_s, 9000 + 20 * _k)
for _k, _s in enumerate([(8, 8), (16, 16), (32, 8)]):
    _lfnst_case(_s, 9400 + 20 * _k, dual=True)


# ----------------------------------------------------------------------------------------------------------------------------------------------------
# transform_types: the DST-7 / DCT-8 bases per size, the implicit pairs of SBT, DCT-2 up to the last kept position
#
# ("mts", w, h, mts_idx), mts_idx = 2 .. 5, w, h = 4 .. 32: mts_idx() is read for luma blocks of at most 32 x 32 (CABACReader.cpp, mts_idx: MTS_INTRA_MAX_CU_SIZE)
#   and selects ( DST-7 | DCT-8 ) per direction (getTrTypes, TrQuant.cpp:330); levels outside the first 16 x 16 are zero (the zero-out of a side of 32), as drawn.
#   A rewrite sets mts_idx and the pair in tr_type together.  Moves: the other type horizontally, the other type vertically.
# ("sbt", w, h, sbt_idx, position): checkAllowedSbt (UnitTools.cpp:3351-3380): inter CUs without CIIP, no side above 64; vertical half from a width of 8,
#   horizontal half from a height of 8, the quarters from 16; position 0 / 1 says which part holds the residual and selects the pair (TrQuant.cpp:366-398; DCT-2
#   where the part has a side above 32).  The split decides the transform units, so it is drawn.  Moves: the other type per direction of the part's pair; for
#   a DCT-2 part its first level changed.
# ("dct2_last", w, h), w, h = 4 .. 64: a DCT-2 block with a level at the last kept position ( min( w, 32 ) - 1, min( h, 32 ) - 1 ).  A rewrite moves the block's
#   levels into a block of the full kept size at the end of the level array and sets the corner.  Move: that level to zero.
# ----------------------------------------------------------------------------------------------------------------------------------------------------
def _luma_tu(d, k):
    """the first transform unit of CU k with a coded luma block, or -1"""
    f = int(d.cu["first_tu"][k])
    for t in range(f, f + int(d.cu["num_tu"][k])):
        if int(d.tu["cbf"][t]) & 1:
            return t
    return -1


def set_tu(d, t, mts_idx=None, tr_type=None, level=None):
    keep = (int(d.tu["mts_idx"][t, 0]), int(d.tu["tr_type"][t, 0]))
    if mts_idx is not None:
        d.tu["mts_idx"][t, 0] = mts_idx
        tr_type = ((1 if (mts_idx - 2) >> 1 else 2) << 2) | (1 if (mts_idx - 2) & 1 else 2)
    if tr_type is not None:
        d.tu["tr_type"][t, 0] = tr_type
    at = None
    if level is not None:
        at = int(d.tu["coef_off"][t, 0]) + level[0]
        old = int(d.coef[at])
        d.coef[at] = level[1](old)

    def undo():
        d.tu["mts_idx"][t, 0], d.tu["tr_type"][t, 0] = keep
        if at is not None:
            d.coef[at] = old
    return undo


def _swap_type(tr_type, vertical):
    """DCT-8 (1) <-> DST-7 (2) in one direction of tr_type = ( vertical << 2 ) | horizontal"""
    hor, ver = tr_type & 3, tr_type >> 2
    return ((3 - ver) << 2 | hor) if vertical else (ver << 2 | (3 - hor))


def _tt_case(kind, shape, seed):
    w, h = shape
    W, H, inside = _sizes(w, h)
    small = 2 if min(w, h) == 4 else 3
    if kind == "mts":
        legal = {("mts", w, h, i) for i in (2, 3, 4, 5)}
        slice_type, tools, kw, n = I, TOOLS_I, dict(INTRA_I, p_mts=0.9, p_lfnst=0.0, p_ts=0.0, p_bdpcm=0.0, p_coded=0.9, p_small_corner=0.3), 1 if inside >= 40 else 2
    elif kind == "sbt":
        legal = {("sbt", w, h, i, p) for i, ok in ((1, w >= 8), (2, h >= 8), (3, w >= 16), (4, h >= 16)) if ok for p in (0, 1)}
        slice_type, tools, kw, n = B, TOOLS_A, dict(p_sbt=0.9, p_intra=0.0, p_ciip=0.0, p_coded=0.9, p_bi=0.5, p_small_corner=0.3), 1 if inside >= 40 else 4
    else:
        legal = {("dct2_last", w, h)}
        slice_type, tools, kw, n = I, TOOLS_I & ~abi.TOOL_LFNST, dict(INTRA_I, p_mts=0.0, p_lfnst=0.0, p_ts=0.0, p_bdpcm=0.0, p_coded=0.9), 1
    specs = [(W, H, (7, 6)[i % 2], seed + i) for i in range(n)]

    def subjects(d):
        cu = d.cu
        out = []
        for k in np.flatnonzero((cu["w"] == w) & (cu["h"] == h) & (cu["tree"] != abi.TREE_CHROMA)):
            t = _luma_tu(d, k)
            if t < 0:
                continue
            m = int(d.tu["mts_idx"][t, 0])
            if kind == "mts" and cu["pred_mode"][k] == abi.PRED_INTRA and not cu["isp_mode"][k] and 2 <= m <= 5:
                out.append((k, t))
            elif kind == "sbt" and cu["pred_mode"][k] == abi.PRED_INTER and cu["sbt_info"][k]:
                out.append((k, t))
            elif kind == "dct2_last" and cu["pred_mode"][k] == abi.PRED_INTRA and not cu["isp_mode"][k] and m == abi.MTS_DCT2 and not cu["lfnst_idx"][k]:
                out.append((k, t))
        return out

    def build(case, spec, state):
        W, H, l2, s = spec
        d, refs = lc.one_picture(W, H, l2, s, tools, ("noise", "checker"), slice_type=slice_type, grid_w=w, grid_h=h, min_cu_log2=small, **kw)
        if kind == "mts":
            q = _Queue(state, "idx", [2, 3, 4, 5], s)
            for k, t in subjects(d):
                set_tu(d, t, mts_idx=q.next())
        elif kind == "dct2_last":
            cw, ch = min(w, 32), min(h, 32)
            extra = []
            at = len(d.coef)
            for n_, (k, t) in enumerate(subjects(d)):
                ow, oh, off = int(d.tu["max_scan_x"][t, 0]) + 1, int(d.tu["max_scan_y"][t, 0]) + 1, int(d.tu["coef_off"][t, 0])
                blk = np.zeros((ch, cw), np.int16)
                blk[:oh, :ow] = d.coef[off:off + ow * oh].reshape(oh, ow)
                blk[ch - 1, cw - 1] = 3 if n_ & 1 else -3
                extra.append(blk.reshape(-1))
                d.tu["coef_off"][t, 0], d.tu["max_scan_x"][t, 0], d.tu["max_scan_y"][t, 0] = at, cw - 1, ch - 1
                at += cw * ch
            d.coef = np.concatenate([d.coef] + extra).astype(np.int16)
        return d, refs

    def instances(d):
        out = []
        for k, t in subjects(d):
            if kind == "mts":
                out.append((k, [("mts", w, h, int(d.tu["mts_idx"][t, 0]))]))
            elif kind == "sbt":
                out.append((k, [("sbt", w, h, int(d.cu["sbt_info"][k]) & 15, int(d.cu["sbt_info"][k]) >> 4)]))
            elif (int(d.tu["max_scan_x"][t, 0]), int(d.tu["max_scan_y"][t, 0])) == (min(w, 32) - 1, min(h, 32) - 1) and d.coef[int(d.tu["coef_off"][t, 0]) + min(w, 32) * min(h, 32) - 1]:
                out.append((k, [("dct2_last", w, h)]))
        return out

    def move(d, k):
        t = _luma_tu(d, k)
        tr = int(d.tu["tr_type"][t, 0])
        if kind == "dct2_last":
            return [lambda: set_tu(d, t, level=(min(w, 32) * min(h, 32) - 1, lambda v: 0))]
        if kind == "sbt" and tr == 0:
            return [lambda: set_tu(d, t, level=(0, lambda v: v + 3))]
        if kind == "mts":
            m = int(d.tu["mts_idx"][t, 0])
            return [lambda: set_tu(d, t, mts_idx=2 + ((m - 2) ^ 1)), lambda: set_tu(d, t, mts_idx=2 + ((m - 2) ^ 2))]
        return [lambda: set_tu(d, t, tr_type=_swap_type(tr, False)), lambda: set_tu(d, t, tr_type=_swap_type(tr, True))]
    CASES.append(Case("transform_types_%s_%dx%d" % (kind, w, h), "transform_types", specs, build, legal, instances, move, luma_only=True))
    CASES[-1].shape = shape


for _k, _s in enumerate([(w, h) for w in SIDES[:4] for h in SIDES[:4]]):
    _tt_case("mts", _s, 9600 + 5 * _k)
for _k, _s in enumerate([s for s in SHAPES if max(s) >= 8]):
    _tt_case("sbt", _s, 9700 + 5 * _k)
for _k, _s in enumerate(SHAPES):
    _tt_case("dct2_last", _s, 9900 + 5 * _k)


FAMILIES = sorted({c.family for c in CASES})


def plane_count(c):
    return 3 if c.cf else 1
