"""The cases of the picture-partitioning tests: tile grids, slice layouts, virtual boundaries and sub-pictures at the ends of what the syntax allows - tiles one
CTU wide and high, a last tile column 8 samples wide, 20 tile columns, raster-scan slices that start in the middle of a tile row (the ALF corner padding),
rectangular slices inside tiles beside a slice of several tiles, 256 slices with headers of their own, virtual boundaries at 8 and size - 8, on tile edges,
beside ALF's own line-buffer boundary and three at the smallest legal spacing, sub-pictures of one CTU.

One table, two users, like tests/limits_cases.py (whose mechanics this reuses): tests/test_oracle_vs_ref_partitions.py pins every input on the CPU (oracle
against the reference classes), tests/test_gpu_partitions.py runs the same inputs through the back-end against the oracle.  A case is a builder
`make() -> (description, reference pictures)` plus a check `present(case, d, refs, stages)`: the structure is there, it sits where the loop filters / the
prediction look, and the oracle's picture changes without it.  `present` works from the description's maps and records and the oracle's stage outputs only.
What it counted goes into Case.found.  (A layout has no "middle of the range": the table is PARTITION_CASES, not limits_cases.CASES.)

Every layout here is one a conforming stream can carry: the generator refuses the others (tools/synth.cpp: VVS_ERR_LAYOUT / VVS_ERR_BOUNDARIES)."""
import numpy as np

import refdrv
import limits_cases as lc
from limits_cases import Case, differ, one_picture
from vvdec_amd import abi, synth
from test_gpu_parity import TOOLS_A

B, I = abi.SLICE_B, abi.SLICE_I
NO_SLICES, NO_TILES = abi.TOOL_NO_LF_ACROSS_SLICES, abi.TOOL_NO_LF_ACROSS_TILES
TOOLS_P = TOOLS_A | abi.TOOL_LMCS | abi.TOOL_LMCS_CSCALE
# intra tools, residuals in most blocks, the loop filters on in nearly every CTU: what a partition boundary cuts is there at every boundary
MIX = dict(p_cclm=0.35, p_mip=0.2, p_isp=0.2, p_coded=0.6, p_coded_chroma=0.6, p_sao=0.9, p_alf_luma=0.95, p_alf_chroma=0.9, p_ccalf=0.8, p_split_scale=1.3)
MIX_B = dict(MIX, p_intra=0.35, p_affine=0.15, p_ciip=0.15, p_bi=0.6, mv_sigma=6.0)
KINDS = ("noise", "steps")

PARTITION_CASES = []


def case(id, family, present, l2, **attrs):
    def reg(make):
        c = Case(id, family, make, present, derive_lfp=True, l2=l2)
        c.__dict__.update(attrs)
        PARTITION_CASES.append(c)
        return make
    return reg


def pictures(id, family, present, W, H, l2, seed, tools, post=None, types=(I, B), **kw):
    """one case per picture type: `id`_i and `id`_b"""
    attrs = {k: kw.pop(k) for k in ("grid", "vbs") if k in kw}
    attrs["layout"] = {k: kw[k] for k in ("tile_col_w", "tile_row_h", "slice_map", "vb_x", "vb_y") if k in kw}
    for t in types:
        @case("%s_%s" % (id, "i" if t == I else "b"), family, present, l2, **attrs)
        def make(t=t):
            d, refs = one_picture(W, H, l2, seed + (1 if t == B else 0), tools, KINDS, slice_type=t, **dict(MIX if t == I else MIX_B, **kw))
            if post:
                post(d, seed, kw)
            return d, refs


# ----------------------------------------------------------------------------------------------------------------------------------------------------
# what present() reads
# ----------------------------------------------------------------------------------------------------------------------------------------------------
def geometry(d):
    l2 = int(d.hdr.log2_ctu)
    S = 1 << l2
    return l2, S, (int(d.hdr.width) + S - 1) >> l2, (int(d.hdr.height) + S - 1) >> l2


def ctu_maps(d):
    """(tile, slice) of every CTU as [ctus_y, ctus_x] arrays"""
    l2, S, cx, cy = geometry(d)
    z = np.zeros((cy, cx), np.int64)
    return (z if d.ctu_tile is None else d.ctu_tile.reshape(cy, cx).astype(np.int64)), (z if d.ctu_slice is None else d.ctu_slice.reshape(cy, cx).astype(np.int64))


def blocked(d, tile, slc, a, b):
    """may the loop filters of CTU a = (y, x) not look into CTU b?  (pps_loop_filter_across_slices / tiles_enabled_flag)"""
    f = int(d.hdr.tool_flags)
    return bool((f & NO_SLICES) and slc[a] != slc[b]) or bool((f & NO_TILES) and tile[a] != tile[b])


def sao_edge(d):
    """per CTU: SAO luma on with an edge class (the classes that look at neighbours)"""
    l2, S, cx, cy = geometry(d)
    return ((d.sao["mode"][:, 0] == 1) & (d.sao["type"][:, 0] < 4)).reshape(cy, cx)


def alf_on(d):
    """per CTU: (luma, a chroma component, a CC-ALF component) on"""
    l2, S, cx, cy = geometry(d)
    e = d.alf["enable"]
    return (e[:, 0] != 0).reshape(cy, cx), ((e[:, 1] != 0) | (e[:, 2] != 0)).reshape(cy, cx), (d.alf["cc_idc"] != 0).any(axis=1).reshape(cy, cx)


def with_flags(d, refs, toggle, flags=0):
    """the oracle's picture with tool flags of the picture header toggled (the records, edge tables included, as they are: what changes is what SAO, ALF and
    CC-ALF may read)"""
    d.hdr.tool_flags ^= toggle
    try:
        return refdrv.oracle_reconstruct(d, refs, flags=flags)
    finally:
        d.hdr.tool_flags ^= toggle


# ----------------------------------------------------------------------------------------------------------------------------------------------------
# tile grids: tiles of one CTU, a last column 8 samples wide, a non-uniform grid, the most columns the syntax allows
# ----------------------------------------------------------------------------------------------------------------------------------------------------
def _tile_grid_present(c, d, refs, st):
    l2, S, cx, cy = geometry(d)
    W, H = int(d.hdr.width), int(d.hdr.height)
    tile, slc = ctu_maps(d)
    cols, rows = c.grid
    assert np.array_equal(tile, synth.tile_of_ctu(cols, rows)) and d.ctu_slice is None
    sizes = np.bincount(tile.reshape(-1))
    found = dict(tiles=len(sizes), one_ctu_tiles=int((sizes == 1).sum()), last_column_samples=W - (cx - 1) * S)
    assert found["one_ctu_tiles"] > 0
    # intra CUs whose neighbour exists in the picture, in another tile: no reference samples, no CCLM template from there (sameSliceAndTile, vvr_prepare.cpp)
    n = dict(left=0, above=0, above_right_only=0, cclm=0)
    for cu in d.cu[(d.cu["pred_mode"] == abi.PRED_INTRA) & (d.cu["tree"] != abi.TREE_CHROMA)]:
        x, y, w, h = int(cu["x"]), int(cu["y"]), int(cu["w"]), int(cu["h"])
        own = tile[y >> l2, x >> l2]
        left = x > 0 and tile[y >> l2, (x - 1) >> l2] != own
        above = y > 0 and tile[(y - 1) >> l2, x >> l2] != own
        ar = y > 0 and x + w < W and not above and tile[(y - 1) >> l2, (x + w) >> l2] != own
        n["left"] += left
        n["above"] += above
        n["above_right_only"] += ar
        n["cclm"] += (left or above or ar) and int(cu["intra_dir"][1]) >= 67
    assert n["left"] > 0 and n["above"] > 0 and n["cclm"] > 0, n
    if len(cols) > 1 and max(rows) > 1:     # (a tile higher than one CTU beside another column: a CU below the tile's first row looks up and right into that column)
        assert n["above_right_only"] > 0, n
    found["intra_cus_with_neighbour_in_another_tile"] = {k: int(v) for k, v in n.items()}
    # chroma residual scaling: the luma neighbourhood of the VPDU, left of and above it
    V = min(S, 64)
    scaled = 0
    for tu in d.tu[(d.tu["cbf"] & 6) != 0]:
        vx, vy = int(tu["x"]) & ~(V - 1), int(tu["y"]) & ~(V - 1)
        own = tile[vy >> l2, vx >> l2]
        scaled += (vx > 0 and tile[vy >> l2, (vx - 1) >> l2] != own) or (vy > 0 and tile[(vy - 1) >> l2, vx >> l2] != own)
    assert scaled > 0 and (int(d.hdr.tool_flags) & abi.TOOL_LMCS_CSCALE)
    found["chroma_scaled_tus_with_vpdu_neighbour_in_another_tile"] = int(scaled)
    # the loop filters at the four sides of a tile
    luma, chroma, cc = alf_on(d)
    sides = [0, 0, 0, 0]
    for y in range(cy):
        for x in range(cx):
            for k, (dy, dx) in enumerate(((0, -1), (0, 1), (-1, 0), (1, 0))):
                if 0 <= y + dy < cy and 0 <= x + dx < cx and tile[y + dy, x + dx] != tile[y, x] and luma[y, x]:
                    sides[k] += 1
    assert all(s > 0 for s in sides), sides
    found["alf_luma_ctus_at_tile_edge_left_right_top_bottom"] = sides
    assert differ(st(0), with_flags(d, refs, NO_TILES)), "pps_loop_filter_across_tiles_enabled_flag changes nothing"
    c.found = found


GRID = ((1, 3, 1, 2, 1), (1, 2, 1, 1))          # 8 x 5 CTUs; the picture width leaves the last column 8 samples wide
pictures("tiles_one_ctu_wide_and_high_ctu32", "tile_grid", _tile_grid_present, 232, 160, 5, 4101, TOOLS_P | NO_TILES, tile_col_w=GRID[0], tile_row_h=GRID[1], grid=GRID)
pictures("tiles_one_ctu_wide_and_high_ctu64", "tile_grid", _tile_grid_present, 456, 320, 6, 4103, TOOLS_P | NO_TILES, tile_col_w=GRID[0], tile_row_h=GRID[1], grid=GRID)
pictures("tiles_20_columns", "tile_grid", _tile_grid_present, 640, 64, 5, 4105, TOOLS_P | NO_TILES, tile_col_w=(1,) * 20, tile_row_h=(1, 1), grid=((1,) * 20, (1, 1)))
pictures("tiles_grid_filters_cross_ctu32", "tile_grid", _tile_grid_present, 232, 160, 5, 4107, TOOLS_P, tile_col_w=GRID[0], tile_row_h=GRID[1], grid=GRID)
pictures("tiles_grid_filters_cross_ctu64", "tile_grid", _tile_grid_present, 456, 320, 6, 4109, TOOLS_P, tile_col_w=GRID[0], tile_row_h=GRID[1], grid=GRID)


# ----------------------------------------------------------------------------------------------------------------------------------------------------
# raster-scan slices that start in the middle of a tile row: the ALF corner padding (alf_clip_of_ctu's flags 16 / 32, vvr_kernels.hip)
# ----------------------------------------------------------------------------------------------------------------------------------------------------
def corner_ctus(d):
    """CTUs whose diagonal neighbour above-left (-> first list) / below-right (second list) lies in another slice while the loop filters may look into the
    CTUs above and left (below and right): AdaptiveLoopFilter's rasterSliceAlfPad"""
    l2, S, cx, cy = geometry(d)
    tile, slc = ctu_maps(d)
    first, last = [], []
    if not (int(d.hdr.tool_flags) & NO_SLICES):
        return first, last
    for y in range(cy):
        for x in range(cx):
            if x > 0 and y > 0 and not blocked(d, tile, slc, (y, x), (y, x - 1)) and not blocked(d, tile, slc, (y, x), (y - 1, x)) and slc[y - 1, x - 1] != slc[y, x]:
                first.append((y, x))
            if x + 1 < cx and y + 1 < cy and not blocked(d, tile, slc, (y, x), (y, x + 1)) and not blocked(d, tile, slc, (y, x), (y + 1, x)) and slc[y + 1, x + 1] != slc[y, x]:
                last.append((y, x))
    return first, last


def alf_stage_alone(c, d, after_sao):
    """-> (description, reference pictures): the layout, boundaries, loop-filter flags and ALF parameters of `d` on a picture whose CUs all copy `after_sao`"""
    h = d.hdr
    tools = abi.TOOL_ALF | abi.TOOL_CCALF | abi.TOOL_DEBLOCK_OFF | (int(h.tool_flags) & (NO_SLICES | NO_TILES))
    lone, _ = one_picture(int(h.width), int(h.height), int(h.log2_ctu), 1, tools, KINDS, slice_type=abi.SLICE_P, **dict(lc.COPY, **c.layout))
    lone.alf, lone.alf_params = d.alf.copy(), d.alf_params
    return lone, {1: after_sao, 2: after_sao}


def _raster_present(c, d, refs, st):
    l2, S, cx, cy = geometry(d)
    tile, slc = ctu_maps(d)
    assert np.array_equal(d.ctu_slice, synth.raster_slices(RASTER_GRID[0], RASTER_GRID[1], RASTER_RUNS)[1])
    first, last = corner_ctus(d)
    # (checked by hand for 4 x 3 tiles of 2 x 2 CTUs and runs (1, 5, 4, 2): tile 5's first CTU and tile 1's last CTU)
    assert (2, 2) in first and (1, 3) in last, (first, last)
    luma, chroma, cc = alf_on(d)
    vx, vy = [int(v) for v in d.hdr.vb_pos_x[:d.hdr.num_ver_vb]], [int(v) for v in d.hdr.vb_pos_y[:d.hdr.num_hor_vb]]
    found = dict(ctus_above_left_in_another_slice=len(first), ctus_below_right_in_another_slice=len(last), with_alf_luma_chroma_ccalf=[0, 0], deciding_samples=[0, 0], deciding_chroma_samples=[0, 0], cut_by_a_virtual_boundary=0)
    final = st(0)
    # the ALF stage on its own: a picture of the same layout whose CUs copy a reference picture - the case's picture after SAO - with the case's ALF parameters, no
    # deblocking, no SAO.  Nothing but ALF and CC-ALF reads its slice map; with the map as it is, it is the case's final picture
    lone, lone_refs = alf_stage_alone(c, d, st(refdrv.STOP_AFTER_SAO))
    assert not differ(refdrv.oracle_reconstruct(lone, lone_refs), final), "the ALF stage alone does not give the case's picture"
    keep = lone.ctu_slice.copy()
    for k, (lst, dy, dx) in enumerate(((first, -1, -1), (last, 1, 1))):
        for (y, x) in lst:
            if not (luma[y, x] and chroma[y, x] and cc[y, x]):       # (all three take the corner flags: alf_clip_of_ctu for luma and for chroma coordinates)
                continue
            found["with_alf_luma_chroma_ccalf"][k] += 1
            found["cut_by_a_virtual_boundary"] += any(x * S < v < (x + 1) * S for v in vx) or any(y * S < v < (y + 1) * S for v in vy)
            # the diagonal neighbour moved into the CTU's own slice, for the ALF stage alone: the 4 x 4 luma block in that corner of the CTU is filtered from other
            # samples, and so are the chroma samples of the corner
            lone.ctu_slice[(y + dy) * cx + x + dx] = slc[y, x]
            other = refdrv.oracle_reconstruct(lone, lone_refs)
            lone.ctu_slice[:] = keep
            y0, x0 = (y * S, x * S) if k == 0 else (min((y + 1) * S, int(d.hdr.height)) - 4, min((x + 1) * S, int(d.hdr.width)) - 4)
            found["deciding_samples"][k] += int((other[0][y0:y0 + 4, x0:x0 + 4] != final[0][y0:y0 + 4, x0:x0 + 4]).sum())
            found["deciding_chroma_samples"][k] += sum(int((other[p][y0 >> 1:(y0 >> 1) + 2, x0 >> 1:(x0 >> 1) + 2] != final[p][y0 >> 1:(y0 >> 1) + 2, x0 >> 1:(x0 >> 1) + 2]).sum()) for p in (1, 2))
    assert min(found["with_alf_luma_chroma_ccalf"]) > 0 and min(found["deciding_samples"]) > 0, found
    if vx or vy:
        assert found["cut_by_a_virtual_boundary"] > 0, found
    assert differ(final, with_flags(d, refs, NO_SLICES)), "pps_loop_filter_across_slices_enabled_flag changes nothing"
    c.found = found


RASTER_GRID, RASTER_RUNS = ((2, 2, 2, 2), (2, 2, 2)), (1, 5, 4, 2)
_RASTER = dict(tile_col_w=RASTER_GRID[0], tile_row_h=RASTER_GRID[1], slice_map=synth.raster_slices(RASTER_GRID[0], RASTER_GRID[1], RASTER_RUNS))
pictures("raster_slices_start_mid_row_ctu32", "raster_slices", _raster_present, 256, 192, 5, 4201, TOOLS_P | NO_SLICES, **_RASTER)
pictures("raster_slices_start_mid_row_ctu64", "raster_slices", _raster_present, 512, 384, 6, 4211, TOOLS_P | NO_SLICES, **_RASTER)
# a virtual boundary of each direction through the two CTUs: the part at the CTU's origin (end) keeps the corner padding, the parts cut off lose it (`& ~16u` / `& ~32u` in
# alf_clip_vb).  (With pps_loop_filter_across_tiles_enabled_flag off as well the corner padding cannot occur: the CTUs above and left then lie in the CTU's own tile, so does
# the diagonal one, and slices inside a tile are bands of CTU rows - a diagonal neighbour in another slice means the CTU above is in another slice too.)
pictures("raster_slices_boundary_through_the_corner_ctus_ctu32", "raster_slices", _raster_present, 256, 192, 5, 4201, TOOLS_P | NO_SLICES, vb_x=(80, 120), vb_y=(48, 80), **_RASTER)
pictures("raster_slices_boundary_through_the_corner_ctus_ctu64", "raster_slices", _raster_present, 512, 384, 6, 4211, TOOLS_P | NO_SLICES, vb_x=(160, 240), vb_y=(96, 160), **_RASTER)


# ----------------------------------------------------------------------------------------------------------------------------------------------------
# rectangular slices inside tiles beside a slice of several tiles; 256 slices
# ----------------------------------------------------------------------------------------------------------------------------------------------------
def _vary(d, seed, kw):
    synth.vary_slices(d, seed, intra_slices=kw.get("intra_slices", 0))


def boundary_kinds(d):
    """pairs of neighbouring CTUs -> (slice boundaries that are no tile boundaries, tile boundaries that are no slice boundaries), and of each those with a SAO edge
    class and ALF luma on in a CTU beside it"""
    l2, S, cx, cy = geometry(d)
    tile, slc = ctu_maps(d)
    edge, (luma, chroma, cc) = sao_edge(d), alf_on(d)
    n = dict(slice_not_tile=[0, 0], tile_not_slice=[0, 0])
    for y in range(cy):
        for x in range(cx):
            for (dy, dx) in ((0, 1), (1, 0)):
                if y + dy >= cy or x + dx >= cx:
                    continue
                a, b = (y, x), (y + dy, x + dx)
                key = "slice_not_tile" if slc[a] != slc[b] and tile[a] == tile[b] else "tile_not_slice" if tile[a] != tile[b] and slc[a] == slc[b] else None
                if key:
                    n[key][0] += 1
                    n[key][1] += bool((edge[a] or edge[b]) and (luma[a] or luma[b]))
    return n


def _rect_present(c, d, refs, st):
    n = boundary_kinds(d)
    assert min(n["slice_not_tile"]) > 0 and min(n["tile_not_slice"]) > 0, n
    assert d.slices is not None and len(d.slices) == 6 and len(set(int(f) for f in d.slices["tool_flags"])) > 1
    final = st(0)
    for flag in (NO_SLICES, NO_TILES):
        assert differ(final, with_flags(d, refs, flag)), "flag %#x changes nothing" % flag
    if int(d.hdr.slice_type) != I:        # the I slice of the B picture
        l2, S, cx, cy = geometry(d)
        in_i = d.slices["slice_type"][d.ctu_slice[(d.cu["y"].astype(int) >> l2) * cx + (d.cu["x"].astype(int) >> l2)]] == I
        assert in_i.any() and (d.cu["pred_mode"][in_i] != abi.PRED_INTER).all() and (d.cu["pred_mode"][~in_i] == abi.PRED_INTER).any()
        n["cus_in_the_i_slice"] = int(in_i.sum())
    c.found = n


RECT_GRID = ((3, 3), (3, 3))
_RECT = dict(tile_col_w=RECT_GRID[0], tile_row_h=RECT_GRID[1], slice_map=synth.rect_slices(RECT_GRID[0], RECT_GRID[1], [(1, 2), (1, 1, 1), "whole", ("join", 2)]))
for _name, _fl in (("no_lf_across_slices", NO_SLICES), ("no_lf_across_tiles", NO_TILES), ("no_lf_across_both", NO_SLICES | NO_TILES)):
    pictures("rect_slices_inside_tiles_%s_ctu32" % _name, "rect_slices", _rect_present, 192, 192, 5, 4301 + _fl % 7, TOOLS_P | _fl, post=_vary, types=(I,), **_RECT)
    pictures("rect_slices_inside_tiles_%s_ctu32" % _name, "rect_slices", _rect_present, 192, 192, 5, 4311 + _fl % 7, TOOLS_P | _fl, post=_vary, types=(B,), intra_slices=0b10, **_RECT)
for _name, _fl in (("no_lf_across_slices", NO_SLICES), ("no_lf_across_tiles", NO_TILES), ("no_lf_across_both", NO_SLICES | NO_TILES)):      # the fused k_sao_alf
    pictures("rect_slices_inside_tiles_%s_ctu64" % _name, "rect_slices", _rect_present, 384, 384, 6, 4321 + _fl % 7, TOOLS_P | _fl, post=_vary, types=(I,), **_RECT)
    pictures("rect_slices_inside_tiles_%s_ctu64" % _name, "rect_slices", _rect_present, 384, 384, 6, 4331 + _fl % 7, TOOLS_P | _fl, post=_vary, types=(B,), intra_slices=0b10, **_RECT)


def _slices_256_present(c, d, refs, st):
    l2, S, cx, cy = geometry(d)
    assert int(d.ctu_slice.max()) + 1 == 256 and len(d.slices) == 256 and len(np.unique(d.ctu_slice)) == 256
    kinds = len(set(int(f) for f in d.slices["tool_flags"]))
    assert kinds > 1
    last = d.ctu_slice[(d.cu["y"].astype(int) >> l2) * cx + (d.cu["x"].astype(int) >> l2)] == 255
    coded = sum(int(((d.tu["cu"] == k) & (d.tu["cbf"] != 0)).sum()) for k in np.flatnonzero(last))
    assert coded > 0
    assert differ(st(0), with_flags(d, refs, NO_SLICES))
    c.found = dict(slices=256, distinct_tool_flags=kinds, coded_tus_in_slice_255=coded)


_S256 = dict(tile_col_w=(1,) * 16, slice_map=synth.rect_slices((1,) * 16, (16,), [(1,) * 16] * 16))
pictures("slices_256", "rect_slices", _slices_256_present, 512, 512, 5, 4331, TOOLS_P | NO_SLICES, post=_vary, **_S256)


# ----------------------------------------------------------------------------------------------------------------------------------------------------
# virtual boundaries at their extreme positions.  With boundaries every picture takes the separate kernels (k_sao, k_alf_luma<VB>, k_alf_chroma(_tile), CC-ALF)
# ----------------------------------------------------------------------------------------------------------------------------------------------------
def _vb_present(c, d, refs, st):
    """per boundary: SAO edge classes on both sides, ALF luma / chroma / CC-ALF in the CTUs it cuts, and the oracle's picture without that boundary.  The picture
    differs for every boundary but one kind, on purpose: a boundary on a tile edge that the filters may not cross anyway (vb_on_tile_edges) decides no sample - SAO
    leaves the same columns alone, ALF clips at the same line - and `present` asserts exactly that (0 samples) instead of a difference.  The case is still worth its
    place: it is the one where alf_clip_vb's `v == cx0` / `v == cx0 + S` arms meet a clipped side of the CTU, and a kernel that got that wrong would differ from the
    oracle (the `<=` -> `<` mutant does)"""
    l2, S, cx, cy = geometry(d)
    W, H = int(d.hdr.width), int(d.hdr.height)
    vx, vy = c.vbs
    assert [int(v) for v in d.hdr.vb_pos_x[:d.hdr.num_ver_vb]] == list(vx) and [int(v) for v in d.hdr.vb_pos_y[:d.hdr.num_hor_vb]] == list(vy)
    edge, (luma, chroma, cc) = sao_edge(d), alf_on(d)
    final = st(0)
    found = {}
    for dr, pos in ((0, vx), (1, vy)):
        for i, v in enumerate(pos):
            lo, hi = (v - 1) >> l2, v >> l2                   # the CTU column / row that holds the sample before the boundary, and the one after it
            pick = (lambda m, k: m[:, k]) if dr == 0 else (lambda m, k: m[k, :])
            sao = [int(pick(edge, lo).sum()), int(pick(edge, hi).sum())]
            cut = sorted({lo, hi})                            # the CTUs the boundary crosses, or the two it lies between
            alf = [int(sum(pick(m, k).sum() for k in cut)) for m in (luma, chroma, cc)]
            assert min(sao) > 0 and min(alf) > 0, (dr, v, sao, alf)
            # without this boundary: another picture
            h = d.hdr
            arr, num = (h.vb_pos_x, "num_ver_vb") if dr == 0 else (h.vb_pos_y, "num_hor_vb")
            keep = list(arr)
            rest = [p for j, p in enumerate(pos) if j != i]
            for j in range(3):
                arr[j] = rest[j] if j < len(rest) else 0
            setattr(h, num, len(rest))
            try:
                other = refdrv.oracle_reconstruct(d, refs)
            finally:
                for j in range(3):
                    arr[j] = keep[j]
                setattr(h, num, len(pos))
            changed = sum(int((a != b).sum()) for a, b in zip(other, final))
            # (on a tile edge the filters may not cross, the boundary says what the tile edge says already: the same columns / rows left alone by SAO, the same clip in ALF)
            tile, slc = ctu_maps(d)
            on_closed_edge = v % S == 0 and blocked(d, tile, slc, (0, v // S) if dr == 0 else (v // S, 0), (0, v // S - 1) if dr == 0 else (v // S - 1, 0))
            assert (changed == 0) if on_closed_edge else (changed > 0), "the boundary at %s = %d decides %d samples" % ("xy"[dr], v, changed)
            found["%s=%d" % ("xy"[dr], v)] = dict(sao_edge_ctus_before_after=sao, alf_luma_chroma_ccalf_ctus=alf, samples_it_decides=changed, on_ctu_boundary=v % S == 0)
    if d.ctu_tile is not None:
        tile, slc = ctu_maps(d)
        on_tile = [v for v in vx if v % S == 0 and tile[0, v // S - 1] != tile[0, v // S]] + [v for v in vy if v % S == 0 and tile[v // S - 1, 0] != tile[v // S, 0]]
        on_ctu = [v for v in vx if v % S == 0 and tile[0, v // S - 1] == tile[0, v // S]] + [v for v in vy if v % S == 0 and tile[v // S - 1, 0] == tile[v // S, 0]]
        assert on_tile and on_ctu and (int(d.hdr.tool_flags) & NO_TILES)
        found["on_tile_edges"], found["on_ctu_edges_inside_tiles"] = len(on_tile), len(on_ctu)
    c.found = found


def _vb_cases(name, W, H, l2, seed, vx, vy, tools=TOOLS_P, **kw):
    pictures("%s_ctu%d" % (name, 1 << l2), "virtual_boundaries", _vb_present, W, H, l2, seed, tools, vb_x=vx, vb_y=vy, vbs=(vx, vy), **kw)


_vb_cases("vb_at_8_and_size_minus_8", 232, 160, 5, 4401, (8, 224), (8, 152))                  # (232 is no multiple of the CTU)
_vb_cases("vb_at_8_and_size_minus_8", 264, 192, 6, 4403, (8, 256), (8, 184))
# tiles 2 + 2 (+ 2) CTUs wide and high: boundaries on the tile edge at two CTUs and on the CTU edge at three / one
_vb_cases("vb_on_tile_edges", 192, 128, 5, 4405, (64, 96), (32, 64), tools=TOOLS_P | NO_TILES, tile_col_w=(2, 2, 2), tile_row_h=(2, 2))
_vb_cases("vb_on_tile_edges", 384, 256, 6, 4407, (128, 192), (64, 128), tools=TOOLS_P | NO_TILES, tile_col_w=(2, 2, 2), tile_row_h=(2, 2))
# eight samples on either side of a CTU edge: beside ALF's line-buffer boundary at ctu - 4
_vb_cases("vb_beside_ctu_rows", 192, 160, 5, 4409, (56, 136), (56, 104))                       # 2 * 32 - 8, 4 * 32 + 8; 2 * 32 - 8, 3 * 32 + 8
_vb_cases("vb_beside_ctu_rows", 320, 256, 6, 4411, (120, 200), (56, 136))                      # 2 * 64 - 8, 3 * 64 + 8; 64 - 8, 2 * 64 + 8
_vb_cases("vb_three_at_smallest_spacing", 160, 128, 5, 4413, (8, 40, 72), (8, 40, 72))
_vb_cases("vb_three_at_smallest_spacing", 256, 200, 6, 4603, (8, 72, 136), (8, 72, 136))      # (200 is no multiple of the CTU)


# ----------------------------------------------------------------------------------------------------------------------------------------------------
# sub-pictures of one CTU and one 8 samples wide, treated as pictures: vectors that leave them through every side
# ----------------------------------------------------------------------------------------------------------------------------------------------------
SUBPIC_MODES = ("uni", "bi", "bdof", "dmvr_bdof", "affine", "affine_4p", "affine_6p", "gpm", "sbtmvp", "ciip")       # k_mc, k_mc_dmvr, k_mc_affine and the CIIP blend


def _subpic_present(c, d, refs, st):
    l2, S, cx, cy = geometry(d)
    tile, slc = ctu_maps(d)
    sp = d.subpics = np.ascontiguousarray(d.subpics)
    assert len(sp) == int(tile.max()) + 1 and (sp["treated_as_pic"] == 1).all() and (sp["lf_across"] == 0).all()
    one_ctu = {k for k in range(len(sp)) if int(sp["x1"][k]) - int(sp["x0"][k]) < S and int(sp["y1"][k]) - int(sp["y0"][k]) < S}
    narrow = {k for k in range(len(sp)) if int(sp["x1"][k]) - int(sp["x0"][k]) == 7}
    assert one_ctu and narrow
    by = {"one_ctu": dict.fromkeys(SUBPIC_MODES, 0), "8_wide": dict.fromkeys(SUBPIC_MODES, 0)}       # (zero counts stay in the record)
    sides = [0, 0, 0, 0]
    for cu in lc._inter(d):
        x, y, w, h = int(cu["x"]), int(cu["y"]), int(cu["w"]), int(cu["h"])
        k = int(tile[y >> l2, x >> l2])
        r = sp[k]
        out = [False] * 4
        for (px, py, mx, my) in lc.cu_vectors(d, cu):
            bw, bh = (w, h) if (px, py) == (x, y) else (8, 8)          # (SbTMVP: per sub-block)
            o = (px + (mx >> 4) < int(r["x0"]), px + bw + ((mx + 15) >> 4) > int(r["x1"]) + 1, py + (my >> 4) < int(r["y0"]), py + bh + ((my + 15) >> 4) > int(r["y1"]) + 1)
            out = [a or b for a, b in zip(out, o)]
        if not any(out):
            continue
        for j in range(4):
            sides[j] += out[j]
        for key in lc._mode_keys(cu):
            if k in one_ctu:
                by["one_ctu"][key] += 1
            if k in narrow:
                by["8_wide"][key] += 1
    assert all(s > 0 for s in sides), sides
    # every mode in both kinds of sub-picture: each fits into 8 samples (BDOF / DMVR: an 8 x 16 CU; GPM: 8 x 8 .. 8 x 32).  With both tools on, a CU that takes DMVR
    # takes BDOF as well (the generator's conditions for DMVR include those for BDOF), so plain "dmvr" cannot occur in these pictures and is not in the list
    for kind in ("one_ctu", "8_wide"):
        assert all(by[kind][m] > 0 for m in SUBPIC_MODES), (kind, by[kind])
    assert not (d.cu["mc_mode"] == abi.MC_DMVR).any()
    pred = st(refdrv.STOP_AFTER_RECO)
    keep = sp["treated_as_pic"].copy()
    sp["treated_as_pic"] = 0
    try:
        other = refdrv.oracle_reconstruct(d, refs, flags=refdrv.STOP_AFTER_RECO)
    finally:
        sp["treated_as_pic"] = keep
    assert differ(pred, other), "sps_subpic_treated_as_pic_flag changes nothing"
    c.found = dict(subpics=len(sp), one_ctu=len(one_ctu), leaving_left_right_top_bottom=sides, cus_leaving_by_mode=by)


_SUB = dict(tile_col_w=GRID[0], tile_row_h=GRID[1], subpics=1 | (1 << 1) | (1 << 3), mv_sigma=60.0, mv_window=500, mv_window_ver=500,
            p_intra=0.1, p_affine=0.25, p_geo=0.15, p_ciip=0.15, p_sbtmvp=0.15, p_bi=0.7, p_coded=0.3, p_coded_chroma=0.3, p_split_scale=1.6, p_boundary_bt=0.5)
# (the quad split at the picture boundary leaves 8 x 8 CUs in the last column - no BDOF, no DMVR; p_boundary_bt gives 8 x 16 and more.  At CTU 32 the grid's rows twice:
# five CTU rows of an 8-wide column hold too few CUs for every mode)
pictures("subpic_one_ctu_and_8_wide_ctu32", "subpictures", _subpic_present, 232, 320, 5, 4501, TOOLS_P, types=(B,), **dict(_SUB, tile_row_h=GRID[1] * 2))
pictures("subpic_one_ctu_and_8_wide_ctu64", "subpictures", _subpic_present, 456, 320, 6, 4512, TOOLS_P, types=(B,), **_SUB)


# the layouts that also run as streams of five pictures through the asynchronous path (tests/test_gpu_partitions.py; on the CPU: the first picture of each)
STREAMS = [
    # name, W, H, log2_ctu, seed, tools, generator parameters, slices with headers of their own
    ("one_ctu_grid", 232, 160, 5, 4601, TOOLS_P | NO_TILES, dict(tile_col_w=GRID[0], tile_row_h=GRID[1]), False),
    ("raster_slices_mid_row", 256, 192, 5, 4602, TOOLS_P | NO_SLICES, _RASTER, False),
    ("rect_slices_inside_tiles", 192, 192, 5, 4603, TOOLS_P | NO_SLICES | NO_TILES, _RECT, True),
    ("vb_at_8_and_size_minus_8", 264, 192, 6, 4604, TOOLS_P, dict(vb_x=(8, 256), vb_y=(8, 184)), False),
]
STREAM_MIX = dict(p_intra=0.3, p_cclm=0.3, p_mip=0.2, p_affine=0.15, p_ciip=0.1, p_coded=0.5, p_coded_chroma=0.5, p_sao=0.8, p_alf_luma=0.9, p_alf_chroma=0.8, p_ccalf=0.7)


# layouts and boundaries the generator must refuse: (name, picture, parameters).  Pictures of 6 x 6 CTUs of 32; T22 = two tile columns and rows of 3 CTUs
def _map(rows):
    return np.array([[int(ch) for ch in r] for r in rows], np.uint16).reshape(-1)


T22 = dict(tile_col_w=(3, 3), tile_row_h=(3, 3))
ILLEGAL = [
    ("tile_widths_do_not_add_up", dict(tile_col_w=(3, 2), tile_row_h=(3, 3))),
    ("tile_heights_exceed_the_picture", dict(tile_col_w=(3, 3), tile_row_h=(3, 3, 1))),
    ("slice_map_of_another_size", dict(T22, slice_map=(synth.SLICES_RECT, np.zeros(35, np.uint16)))),
    ("slice_index_unused", dict(T22, slice_map=(synth.SLICES_RECT, _map(["000222"] * 6)))),
    ("raster_slice_of_half_a_tile", dict(T22, slice_map=(synth.SLICES_RASTER, _map(["000111"] * 2 + ["222111"] + ["222333"] * 3)))),
    ("raster_slices_not_in_tile_order", dict(T22, slice_map=(synth.SLICES_RASTER, _map(["111000"] * 3 + ["222222"] * 3)))),
    ("raster_slice_of_tiles_that_are_not_consecutive", dict(T22, slice_map=(synth.SLICES_RASTER, _map(["000111"] * 3 + ["222000"] * 3)))),
    ("rect_slice_that_is_no_rectangle", dict(T22, slice_map=(synth.SLICES_RECT, _map(["000000"] * 3 + ["000111"] * 3)))),
    ("rect_slice_of_a_tile_and_a_half", dict(T22, slice_map=(synth.SLICES_RECT, _map(["000000"] * 4 + ["111222"] * 2)))),
    ("rect_slice_of_half_ctu_rows", dict(T22, slice_map=(synth.SLICES_RECT, _map(["001222"] * 3 + ["333444"] * 3)))),
    ("rect_slices_in_a_tile_side_by_side", dict(T22, slice_map=(synth.SLICES_RECT, _map(["011222"] * 3 + ["333444"] * 3)))),
    ("rect_slices_numbered_out_of_order", dict(T22, slice_map=(synth.SLICES_RECT, _map(["111000"] * 3 + ["222333"] * 3)))),
    ("rect_bands_numbered_bottom_up", dict(T22, slice_map=(synth.SLICES_RECT, _map(["111222"] * 1 + ["000222"] * 2 + ["333444"] * 3)))),
    ("slice_map_without_a_mode", dict(T22, slice_map=(0, _map(["000111"] * 3 + ["222333"] * 3)))),
    ("boundary_not_a_multiple_of_8", dict(vb_x=(20,))),
    ("boundary_outside_the_picture", dict(vb_y=(192,))),
    ("boundaries_descending", dict(vb_x=(96, 40))),
    ("boundaries_closer_than_one_ctu", dict(vb_y=(40, 64))),
    ("boundaries_equal", dict(vb_x=(64, 64))),
    ("four_boundaries", dict(vb_x=(8, 40, 72, 104))),
]
LEGAL = [
    ("raster", dict(T22, slice_map=(synth.SLICES_RASTER, _map(["000111"] * 3 + ["111222"] * 3)))),
    ("rect_bands_and_joined_tiles", dict(T22, slice_map=(synth.SLICES_RECT, _map(["000111"] + ["000222"] * 2 + ["333333"] * 3)))),
    ("rect_tiles_joined_downwards", dict(T22, slice_map=(synth.SLICES_RECT, _map(["000111"] * 6)))),
    ("boundaries_one_ctu_apart", dict(vb_x=(8, 40, 72), vb_y=(152, 184))),
]
