// vvdec_amd/csrc/vvr_device.h — device-side view shared by the HIP kernels and the host scheduler (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <utility>
#include "../../include/vvr.h"

typedef int16_t pel_t;

// One picture's planes in HBM.  Rows are 128-byte aligned (stride in samples is a multiple of 64) so that a wavefront
// reading 64 consecutive samples touches exactly one or two 128-B lines.  No border margins: reference reads clamp
// their coordinates, which equals reading the reference decoder's border-extended picture (Picture.cpp:400-518).
struct DevPlanes {
  pel_t* p[3];
  int    stride[3];
  int    w[3], h[3];
};

// Work items built by the host glue (vvr_prepare) from the CU/TU records ---------------------------------------------

// One motion-compensation tile: at most 16x16 luma samples (+ the co-located 8x8 chroma samples) of one inter CU.
// 16x16 is the unit VVC itself uses for DMVR/BDOF processing (DMVR_SUBCU 16x16, MAX_BDOF_APPLICATION_REGION 16).
#define MC_ITEM_SUBBLOCK 1     /* SbTMVP: the tile is one 8x8 sub-block, motion from the motion field */
struct McItem {
  uint16_t x, y;       // luma position
  uint8_t  w, h;       // luma size: 4, 8 or 16
  uint16_t flags;      // MC_ITEM_*
  uint32_t cu;         // index into the CU array
  // plain (k_mc) tiles are self-contained: the kernel starts its reference fetch after ONE dependent load (this record) instead of
  // item -> CU -> motion field; GPM tiles still read their CU
  int32_t  mv[2][2];   // motion vectors of the two lists (1/16 sample), unclipped
  int8_t   ref[2];     // reference indices (-1: list not used)
  uint8_t  bcw;        // BCW weight index (2 = equal weights)
  uint8_t  clipW4;     // 0: the MV clipping refers to the CU's width; else the width / 4 of the block it refers to (SbTMVP under reference wrap-around: the joined piece)
  uint16_t clipX, clipY;   // position the MV clipping refers to (the CU; for SbTMVP the sub-block itself or, under reference wrap-around, the joined piece it belongs to)
};
// An inter CU whose tiles the DEVICE writes (k_expand_mc): the host only counts the tiles of such a CU - plain, BDOF and DMVR tiles are a function of
// the CU record alone (SbTMVP and affine tiles carry motion of the motion field, which stays on the host: those the host writes itself)
struct McCuRef { uint32_t cu; uint32_t first; };      // index into the CU array; bits 30..31: list (0 plain, 1 BDOF, 2 DMVR), bits 0..29: index of the CU's first tile in that list's device-written part
#define MC_ITEM_UNI   2    /* one prediction only: a single list, or identical motion in both (xCheckIdenticalMotion) */
#define MC_ITEM_HPEL  4    /* half-sample AMVR: alternative luma half-sample filter */
#define MC_ITEM_GEO   8
#define MC_ITEM_AFFINE 16  /* (tiles of k_mc_rpr only) affine CU: sub-block MVs like the tiles of k_mc_affine */

// One transform block that carries a residual.
struct TbItem {
  uint32_t tu;         // index into the TU array
  uint8_t  comp;       // component the coded levels belong to
  uint8_t  mode;       // TB_ADD: reco += residual (inter CU, prediction already in the picture); TB_STORE: write residual plane
  uint8_t  ict;        // 0, or 4 + ICT mode (-3..3 -> 1..7): joint Cb-Cr, the item writes both chroma blocks
  uint8_t  pad;        // TB_P_*: what k_itrans must know of the CU before it has the CU record (it asks for the record, the levels and the basis rows at once)
};
enum { TB_ADD = 0, TB_STORE = 1 };
enum { TB_P_CUGEOM = 1 /* chroma block of an ISP CU: position and size are the CU's */, TB_P_BDPCM = 2 /* BDPCM: every level of the block is coded */,
       TB_P_LFNST = 4 /* the CU applies LFNST to this component: cu.lfnst_idx > 0 && ( cu.tree != VVR_TREE_JOINT || comp == 0 ) */ };

// Everything k_itrans needs to know of a transform block, in one 16-byte record per TbItem (same index, an array of its own per size class): what the kernel used to
// chase item -> TU record -> CU record -> slice map at the head of every block.  A pure function of the picture's own records (tb_record below), written on the
// device by prep_tb_records (a section of k_prep, the picture's first launch, in front of the waits for the reference pictures) into room behind the uploaded image.
struct TbRec {
  uint32_t coef;       // offset of the block's level corner in the coefficient stream
  uint16_t x, y;       // position in samples of the component (chroma of an ISP CU: the CU's)
  uint32_t a;          // log2 width (3 bits) | log2 height << 3 | comp << 6 | mode << 8 | ict << 9 (as TbItem) | mts_idx << 12 | tr_type << 15 (4 bits) | BDPCM direction << 19 (2)
                       // | slice: dependent quantisation << 21 | slice: scaling lists on << 22 | scaling-list type << 23 (3) | TB_P_LFNST << 26
                       // | LFNST set << 27 (2) | LFNST index - 1 << 29 | LFNST output transposed << 30
  uint32_t b;          // max_scan_x (8 bits) | max_scan_y << 8 | QP << 16 (8 bits, signed)
};
__host__ __device__ inline int tbr_lw( const TbRec& r )        { return (int) ( r.a & 7 ); }
__host__ __device__ inline int tbr_lh( const TbRec& r )        { return (int) ( ( r.a >> 3 ) & 7 ); }
__host__ __device__ inline int tbr_comp( const TbRec& r )      { return (int) ( ( r.a >> 6 ) & 3 ); }
__host__ __device__ inline int tbr_mode( const TbRec& r )      { return (int) ( ( r.a >> 8 ) & 1 ); }
__host__ __device__ inline int tbr_ict( const TbRec& r )       { return (int) ( ( r.a >> 9 ) & 7 ); }
__host__ __device__ inline int tbr_mts( const TbRec& r )       { return (int) ( ( r.a >> 12 ) & 7 ); }
__host__ __device__ inline int tbr_tr_type( const TbRec& r )   { return (int) ( ( r.a >> 15 ) & 15 ); }
__host__ __device__ inline int tbr_bdpcm( const TbRec& r )     { return (int) ( ( r.a >> 19 ) & 3 ); }
__host__ __device__ inline bool tbr_dep_quant( const TbRec& r ) { return ( r.a >> 21 ) & 1; }
__host__ __device__ inline bool tbr_sl_on( const TbRec& r )    { return ( r.a >> 22 ) & 1; }
__host__ __device__ inline int tbr_list_type( const TbRec& r ) { return (int) ( ( r.a >> 23 ) & 7 ); }
__host__ __device__ inline bool tbr_lfnst( const TbRec& r )    { return ( r.a >> 26 ) & 1; }
__host__ __device__ inline int tbr_lfnst_set( const TbRec& r ) { return (int) ( ( r.a >> 27 ) & 3 ); }
__host__ __device__ inline int tbr_lfnst_idx( const TbRec& r ) { return (int) ( ( r.a >> 29 ) & 1 ); }
__host__ __device__ inline bool tbr_lfnst_transposed( const TbRec& r ) { return ( r.a >> 30 ) & 1; }
__host__ __device__ inline int tbr_scan_x( const TbRec& r )    { return (int) ( r.b & 0xff ); }
__host__ __device__ inline int tbr_scan_y( const TbRec& r )    { return (int) ( ( r.b >> 8 ) & 0xff ); }
__host__ __device__ inline int tbr_qp( const TbRec& r )        { return (int) (int8_t) ( ( r.b >> 16 ) & 0xff ); }

__host__ __device__ inline int tbr_ilog2( int v ) { int l = 0; while( v > 1 ) { v >>= 1; l++; } return l; }
// the record of item `it`; sliceFlags: the tool switches that hold in the slice of the TU's top-left luma sample (the picture's where it has no slice headers)
__host__ __device__ inline TbRec tb_record( const TbItem& it, const vvr_tu& tu, const vvr_cu& cu, uint32_t sliceFlags )
{
  const int comp = it.comp, csh = comp ? 1 : 0;
  int bw = tu.w >> csh, bh = tu.h >> csh, bx = tu.x >> csh, by = tu.y >> csh;
  if( it.pad & TB_P_CUGEOM ) { bw = cu.w >> 1; bh = cu.h >> 1; bx = cu.x >> 1; by = cu.y >> 1; }      // (chroma of an ISP CU)
  const int bdpcm = ( it.pad & TB_P_BDPCM ) ? ( comp ? cu.bdpcm[1] : cu.bdpcm[0] ) : 0;
  const int listType = ( cu.pred_mode == VVR_PRED_INTRA ? 0 : 3 ) + comp;          // (getScalingListType: intra / inter x component)
  uint32_t lf = 0;
  if( it.pad & TB_P_LFNST )
  {
    // the LFNST set and whether its output is transposed, from the intra mode (TrQuant.cpp:201-237): planar for MIP, the luma mode for a chroma block
    // predicted from luma, wide angles mapped by the block's shape (PU::getWideAngIntraMode, UnitTools.cpp:617 - the CU's shape for the partitions of an ISP CU)
    int mode;
    if( ( cu.flags & VVR_CU_MIP ) && comp == 0 ) mode = 0;
    else if( comp && cu.intra_dir[1] >= 67 ) mode = cu.lfnst_intra_mode;
    else mode = cu.intra_dir[comp ? 1 : 0];
    const int w = ( cu.isp_mode && !comp ) ? cu.w : bw, h = ( cu.isp_mode && !comp ) ? cu.h : bh;
    if( mode >= 2 )
    {
      const int dl = tbr_ilog2( w ) - tbr_ilog2( h ), d = dl < 0 ? -dl : dl;
      const int modeShift = d == 0 ? 0 : d == 1 ? 6 : d == 2 ? 10 : d == 3 ? 12 : d == 4 ? 14 : 15;
      if( w > h && mode < 2 + modeShift ) mode += 65;
      else if( h > w && mode > 66 - modeShift ) mode -= 67;
    }
    const int lm = mode < 0 ? mode + 14 + 67 : mode >= 67 ? mode + 14 : mode;
    const bool transpose = ( lm >= 67 && lm >= 67 + 14 ) || ( lm < 67 && lm > 34 );
    // g_lfnstLut (Rom.cpp): 0 for planar / DC and the LM modes, 1 / 2 / 3 / 2 / 1 over the angles
    const int set = lm < 2 ? 0 : lm < 13 ? 1 : lm < 24 ? 2 : lm < 45 ? 3 : lm < 56 ? 2 : lm < 95 ? 1 : 0;
    lf = 1u | ( (uint32_t) set << 1 ) | ( (uint32_t) ( ( cu.lfnst_idx - 1 ) & 1 ) << 3 ) | ( transpose ? 16u : 0u );
  }
  TbRec r;
  r.coef = tu.coef_off[comp]; r.x = (uint16_t) bx; r.y = (uint16_t) by;
  r.a = (uint32_t) tbr_ilog2( bw ) | ( (uint32_t) tbr_ilog2( bh ) << 3 ) | ( (uint32_t) comp << 6 ) | ( (uint32_t) ( it.mode & 1 ) << 8 ) | ( (uint32_t) ( it.ict & 7 ) << 9 )
      | ( (uint32_t) ( tu.mts_idx[comp] & 7 ) << 12 ) | ( (uint32_t) ( tu.tr_type[comp] & 15 ) << 15 ) | ( (uint32_t) bdpcm << 19 )
      | ( ( sliceFlags & VVR_TOOL_DEP_QUANT ) ? 1u << 21 : 0u ) | ( ( sliceFlags & VVR_TOOL_SCALING_LIST ) ? 1u << 22 : 0u ) | ( (uint32_t) listType << 23 ) | ( lf << 26 );
  r.b = (uint32_t) tu.max_scan_x[comp] | ( (uint32_t) tu.max_scan_y[comp] << 8 ) | ( (uint32_t) (uint8_t) tu.qp[comp] << 16 );
  return r;
}

// One intra-predicted transform block (decode order inside its CTU).  The reference-sample availability counts are the
// m_neighborSize[] values IntraPrediction::xFillReferenceSamples derives by walking the CU/TU tree (IntraPrediction.cpp:1104-1139);
// that walk is host glue here (vvr_prepare), the kernel only consumes the counts.
#define IT_F_RESI     1
#define IT_F_BDPCM_H  2
#define IT_F_MIP      8      /* luma: matrix-based intra prediction: mode = matrix index, bit 4 = transposed */
#define IT_F_ISP      6   /* both BDPCM bits (never together otherwise): luma intra sub-partition; IntraItem::tu then holds x - cuX | ( y - cuY ) << 6
                             | log2 cuW << 12 | log2 cuH << 15 | vertical split << 18 | residual flags of the partitions of a group << 19 (4 bits) | group << 23 (1: two 2-wide, 2: four 1-wide partitions) */
#define IT_MODE_RESI_ADD 255 /* mode value: no prediction, the (LMCS-scaled) residual is added to the inter prediction already in the picture */
#define IT_MODE_IBC      254 /* mode value: intra block copy, the prediction is a copy of reconstructed samples of this picture; IntraItem::tu = dx & 0xffff | dy << 16 (component samples) */
#define IT_F_CSCALE   8      /* chroma: LMCS chroma residual scaling applies to the residual */
#define IT_F_BDPCM_V  4      /* bits 4..5: multi-reference-line index; bits 6..7: CIIP intra weight (0 = ordinary intra block) */
struct IntraItem {        // 16 bytes, self-contained: the kernel never touches the CU/TU records on its serial path
  uint16_t x, y;          // block position in the component plane
  uint8_t  lw, lh;        // log2 size
  uint8_t  mode;          // 0 planar, 1 DC, 2..66 angular (before the wide-angle remap)
  uint8_t  flags;         // IT_F_*
  uint8_t  nTL;           // bit 0: top-left reference sample available; bits 1..3: row part of the block this item predicts, bits 4..5: log2( parts )
                          // (a block of more than IT_SPLIT_SAMPLES samples is predicted by 2, 4 or 8 wavefronts, each a band of rows: one item per band)
  uint8_t  nA, nL;        // available units (4 luma samples): above incl. above-right, left incl. below-left
  uint8_t  comp;          // bits 0..1: component; bits 2..7: `indep` - the block reads nothing that the `indep` blocks before it in its unit produce
                          // (it starts when every block of the unit up to index - indep - 1 is done)
  uint32_t tu;
};
#define IT_PART( it )    ( ( (it).nTL >> 1 ) & 7 )
#define IT_LPARTS( it )  ( ( (it).nTL >> 4 ) & 3 )
#define IT_COMP( it )    ( (it).comp & 3 )
#define IT_INDEP( it )   ( (it).comp >> 2 )
#define IT_PART_SAMPLES 1024   /* samples of an item whose residual is kept in the wavefront's LDS scratch (larger items - MIP, CCLM, IBC blocks that are not split - read it from the residual plane) */
#define IT_SPLIT_SAMPLES 256   /* ordinary prediction modes: a block of more samples becomes 2, 4 or 8 items (bands of rows), so that a wavefront predicts a band in one round of four samples per lane */
#define IT_MAX_LPARTS 3

// One unit of the intra stage (blocks of one component inside one CTU that read reference samples from each other, or a group of such
// clusters at the same dependency depth), processed by one workgroup.
#define VVR_INTRA_MAX_DEPS 26
struct IntraUnit {
  uint32_t ent;           // (component << 24) | CTU address; bit 29: has blocks with LMCS chroma residual scaling; bit 30: another unit waits for this one (it must publish its flag)
  uint32_t i0, i1;        // item range
  uint32_t bbox;          // (whole-CTU units only) part of the CTU tile the unit's blocks read: y0 | y1 << 8 | c0 << 16 | c1 << 24 (rows from CTU top - 3, 16-byte chunks from CTU left - 8, chunk + 1)
  uint32_t ndeps;
  uint32_t deps[VVR_INTRA_MAX_DEPS];   // tickets (= indices into the unit table) this unit waits for
  uint32_t iA;                         // [i0, iA): IT_MODE_RESI_ADD items (no mutual dependencies, done first and in parallel); 32 dwords
};

struct PicDev {         // everything a kernel needs about one picture (passed by value)
  vvr_pic_header     hdr;
  const vvr_cu*      cu;
  const vvr_tu*      tu;
  const int16_t*     coef;
  const vvr_motion*  affMotion;      // motion of the 4x4 sub-blocks of the affine tiles: 16 entries (4 x 4) per tile, first entry = McItem::mv[0][0]
  const vvr_lfp*     lfp[2];
  const vvr_sao_ctu* sao;
  const vvr_alf_ctu* alf;
  const vvr_alf_params* alf_params;
  const vvr_lmcs_params* lmcs;       // LMCS tables (NULL when off)
  const vvr_scaling_list* scaling;   // explicit scaling lists (NULL unless VVR_TOOL_SCALING_LIST)
  const vvr_wp_params*   wp;         // explicit weighted prediction table (NULL unless VVR_TOOL_WP on a P / B picture)
  const uint16_t*    ctuSlice;       // slice / tile index of every CTU (NULL: one slice / one tile): where SAO and ALF stop when the picture says so
  const uint16_t*    ctuTile;
  const vvr_slice_header* slices;    // headers of the slices (indexed by ctuSlice), NULL: every slice takes hdr's values; alf_params / wp then are arrays
  int                numAlfSets, numWpSets;
  const vvr_rpr_params* rpr;         // reference picture resampling: how the picture sees its reference pictures (NULL: none is scaled)
  const vvr_subpic*  subpics;        // sub-pictures (NULL: the picture is its only sub-picture) and the sub-picture of every CTU: MC of a CU in a sub-picture
  const uint16_t*    ctuSubpic;      // treated as a picture stays inside it; SAO / ALF of a CTU whose sub-picture says so do not look into other sub-pictures
  const uint32_t*    csVpdu;         // LMCS chroma residual scaling, per VPDU: x | y << 13 | hasLeft << 26 | hasAbove << 27 of the luma neighbourhood the factor is averaged over
  vvr_motion*        colMotion;      // collocated motion of the picture (pinned host memory, device-mapped; NULL unless VVR_TOOL_COL_MOTION): the DMVR kernel patches it
  int                colStride;      // records per row = ( w4 + 1 ) / 2
  int                vpdusX, vpduLog2;
  int                w4, h4, ctus_x, ctus_y;
  const TbRec*       tbRec[3];       // the records of the transform blocks, one per TbItem of the size class (written by k_prep: launch_itrans hands its class's to the kernel)
  int                numTb[3];       // transform blocks per size class (the records of tbRec): the launch of the 16 class takes the 32 class along (VVR_SHARED_ITRANS_LAUNCH)
};

// Build-time switch: 1 - a picture with transform blocks of the 16 and of the 32 class runs both in ONE launch (launch_itrans for the 16 class; the caller makes no
// call for the 32 class); 0 - a launch per class, as before (-DVVR_SHARED_ITRANS_LAUNCH=0: to measure one against the other from one tree).  A picture with one of
// the two classes only takes that class's kernel either way.
#ifndef VVR_SHARED_ITRANS_LAUNCH
#define VVR_SHARED_ITRANS_LAUNCH 1
#endif

struct RefSet { const pel_t* p[2 * VVR_MAX_REFS][3]; };   // reference planes indexed [list * 16 + refIdx][comp]; geometry = the current picture's

// kernel launchers (vvr_kernels.hip) ----------------------------------------------------------------------------------
void launch_mc     ( hipStream_t s, const PicDev& pic, const RefSet& refs, DevPlanes reco, const McItem* items, int numItems, const McItem* items2, int numItems2, int bdof );      // tiles of two arrays (host-written, device-written) in one launch
void launch_itrans ( hipStream_t s, const PicDev& pic, DevPlanes reco, DevPlanes resi, const TbItem* items, int numItems, int sizeClass );
inline bool itrans_shared_launch( const PicDev& pic ) { return VVR_SHARED_ITRANS_LAUNCH && pic.numTb[0] > 0 && pic.numTb[1] > 0; }      // the call for the 16 class launches the 32 class too
// the deblocking edge parameters of the picture from its CU / TU records (vvr_lf_init.h): cell maps, motion of sub-block CUs, one thread per cell and direction
void launch_lf_init( hipStream_t s, const PicDev& pic, uint32_t numCu, uint32_t numTu, struct LfCell* cell, struct LfCell* cellC, struct LfMv* mv, uint32_t* ref, const struct LfSbCell* sbCells, int numSbCells, vvr_lfp* out0, vvr_lfp* out1 );
void launch_deblock( hipStream_t s, const PicDev& pic, DevPlanes reco, int dir );
void launch_deblock_tile( hipStream_t s, const PicDev& pic, DevPlanes src, DevPlanes dst, int dir, bool lmcs );      // one direction out of place (tiles); vertical edges: inverse LMCS in the load
void launch_sao    ( hipStream_t s, const PicDev& pic, DevPlanes src, DevPlanes dst );
void launch_alf    ( hipStream_t s, const PicDev& pic, DevPlanes src, DevPlanes dst );
bool sao_alf_fused ( const PicDev& pic );      // SAO + ALF in one pass (launch_sao_alf) apply to this picture; else launch_sao, launch_alf
void launch_sao_alf( hipStream_t s, const PicDev& pic, DevPlanes src, DevPlanes dst, bool sao, bool alf );
void launch_lmcs   ( hipStream_t s, const PicDev& pic, DevPlanes reco, int inverse );
void launch_copy_planes( hipStream_t s, DevPlanes src, DevPlanes dst );
void launch_copy_bytes( hipStream_t s, const void* src, void* dst, size_t bytes );
void launch_output_window( hipStream_t s, const pel_t* src, int stride, int w, int h, int bytesPerSample, void* dst );      // window rows packed back to back, 1 or 2 bytes per sample
void launch_plane_hash_rows( hipStream_t s, const pel_t* plane, int stride, int w, int h, int two, int crcMode, uint32_t* out );   // per row: checksum share / CRC piece
// rescaled output (sampleRateConvCore, Buffer.cpp:235-318): a window of w x h samples resampled to outW x outH, packed like launch_output_window.
// per direction refPos( i ) = ( i * step + add ) >> shift, step = scale << cs (vvr_output.inc, rescale_axis); luma: the 8-tap DCTIF, else the 4-tap one
struct RescaleParams
{
  const pel_t* src; int stride, w, h, outW, outH;
  int stepX, stepY, addX, addY, shiftX, shiftY;
  int luma, maxVal, bytesPerSample;
};
// The regions of a batch (vvr_output_submit_batch): blockIdx.z of k_rescale, k_output_resample and k_output_resample_h.  Region z reads the plane
// at p.src + srcOff[3 * z + comp] samples (srcOff: a table in device memory, three words per region - the region's origin in the three planes;
// NULL: p.src), stores its rows at dst + z * dstStep bytes and keeps the horizontal results of the two-launch form at scratch + z * hStep words.
// The default is the single request: one region, no table, no steps.
struct PlaneRegions
{
  int count = 1, comp = 0;
  const uint32_t* srcOff = nullptr;
  size_t dstStep = 0, hStep = 0;
};
void launch_rescale( hipStream_t s, const RescaleParams& p, void* dst, const PlaneRegions& rg = PlaneRegions() );
// antialiased resampling (vvr_set_output_resampling, the definition: vvr.h; k_output_resample): a window of w x h samples to outW x outH, stored
// like launch_rescale's.  tabX / tabY: the tap table of an axis in device memory, built on the host from the integer definition - m words
// first | count << 16, one per output sample, then tapsX (tapsY) x m int16 weights tap-major: weight t of output sample i at [ t * m + i ],
// 0 behind a sample's count.  tapsX / tapsY: the largest count of the axis.  Every tap lies inside the plane (first >= 0, first + count <= n).
struct ResampleParams
{
  const pel_t* src; int stride, w, h, outW, outH;
  const uint32_t* tabX; const uint32_t* tabY; int tapsX, tapsY;
  int maxVal, bytesPerSample;
};
// a plane that shrinks by more than 4 vertically takes two launches - k_output_resample_h into `scratch`, h x outW 32-bit words, then the vertical
// pass over those (vvr_kernels.hip) - every other plane one, and no scratch
static inline bool resample_two_launches( int h, int outH ) { return h > 4 * outH; }
void launch_output_resample( hipStream_t s, const ResampleParams& p, void* dst, void* scratch, const PlaneRegions& rg = PlaneRegions() );
// film grain synthesis at the output (FilmGrainImpl::add_grain_block, FilmGrainImpl.cpp:126-324) over a window of every component, packed like
// launch_output_window into dst + dstOff[c].  words: one random word per 16x16 luma block of the window, nbx per band (vvr_output.inc, grain_words);
// bank: the device copy of the context's vvr_film_grain_bank
struct FilmGrainParams
{
  const pel_t* src[3]; int stride[3], w[3], h[3]; size_t dstOff[3];
  const vvr_film_grain_bank* bank; const uint32_t* words; int nbx;
  int numComp, bs, scaleShift, bytesPerSample;
};
void launch_film_grain( hipStream_t s, const FilmGrainParams& p, void* dst );
// a frame of the output queue (vvr_output_submit): the windows of up to three planes, one launch, stored into dst + dstOff[c] (256-byte aligned) with
// the rows back to back in `format` (VVR_OUT_*): 2 bytes or 1 byte per sample, or four samples in five bytes ( s << shift, 10 bits each;
// w[c] a multiple of 4 then ).  A plane with w[c] == 0 is not part of the launch.  The launch may write up to 31 bytes of padding behind a plane.
// The semi-planar formats (VVR_OUT_NV12: 1 byte per sample; VVR_OUT_P010: 2 bytes, s << shift) have two output planes: plane 0 the luma window,
// plane 1 the chroma windows src[1], src[2] (w[1] / 2 samples wide each, stride[1], stride[2]) interleaved Cb0, Cr0, Cb1, ... into rows of w[1]
// samples, h[1] of them; w[2] is 0.
// direct[c] != NULL: plane c is stored there (32-byte aligned memory of the caller's) instead of dst + dstOff[c], and not a byte behind the
// plane's last sample is written.
struct OutputFrameParams
{
  const pel_t* src[3]; int stride[3], w[3], h[3]; size_t dstOff[3];
  uint8_t* direct[3];
  int first[3];      // (set by the launcher: first workgroup of every plane)
  int format, shift;
};
void launch_output_frame( hipStream_t s, OutputFrameParams p, void* dst );
// the 9 / 10 -> 8 bit reduction of the byte-per-sample Y'CbCr formats (vvr_set_output_narrowing, the definition: vvr.h): byte =
// min( 255, ( min( v, maxVal ) + a ) >> s ).  cell[r]: the additive constants of row parity r of the 2 x 2 cell with the phase folded in, the one of
// an even column in the low, of an odd column in the high 16 bits (TRUNCATE: 0; ROUND: ( 1 << ( s - 1 ) ) * 0x10001; DITHER: the matrix)
struct NarrowArgs { int s, maxVal; uint32_t cell[2]; };
// VVR_OUT_PLANAR8 / VVR_OUT_NV12 of a context of 9 or 10 bits (k_output_narrow): p as launch_output_frame takes it, the reduction at the store
void launch_output_narrow( hipStream_t s, OutputFrameParams p, NarrowArgs na, void* dst );
// a frame of the output queue as R'G'B' (planar VVR_OUT_RGB8 / _RGB16 / _RGBF16 / _RGBF32 or one interleaved plane, the definition: vvr.h): one 4:2:0 frame of w x h luma samples
// (even; the chroma planes w / 2 x h / 2), chroma brought to the luma grid by the 4-tap DCTIF at the two phases `collocated` selects per direction
// (taps clamped to the frame), then the Q14 matrix.  Three planes of w x h samples (or one of w x h pixels) leave, rows back to back, into dst + dstOff[c] (256-byte
// aligned) or direct[c] (32-byte aligned memory of the caller's); nothing behind a plane's last sample is written in either.
struct OutputRgbParams
{
  const pel_t* src[3]; int stride[3], w, h; size_t dstOff[3];
  uint8_t* direct[3];
  int format, collocated;
  int maxVal, yoff, coff;      // 2^bd - 1; 16 << ( bd - 8 ) or 0; 2^( bd - 1 )
  int cy, rv, gu, gv, bu, maxOut;      // the Q14 coefficients (vvr_output.inc, rgb_coefficients), 2^od - 1
  float inv;                   // VVR_OUT_RGBF16: float32( 1 ) / float32( 2^bd - 1 ); under a transform float32( 1 ) / float32( 65535 )
  // the colour transform (vvr_set_output_transform, the definition: vvr.h); xform == NULL: none.  xform: the device copy of the context's
  // vvr_output_transform (lin and enc are read from it; 8-byte aligned); xm: its matrix, as kernel arguments.  The matrix above runs at od = bd
  // then, whatever the format.
  const vvr_output_transform* xform; int xm[3][3];
  // the interleaved formats (VVR_OUT_RGBA8 ... _RGBA16F: one plane of pixels, dstOff[0] / direct[0]) and VVR_OUT_RGBF32 (three planes).  format is
  // the class the kernel is compiled for - VVR_OUT_RGBA8 also serves _BGRA8, VVR_OUT_RGB24 also _BGR24 - and swapRB exchanges R and B ahead of
  // the store.  nscale, nbias: the normalisation of VVR_OUT_RGBF32 (vvr_set_output_normalisation, the definition: vvr.h), out = v * nscale[c] + nbias[c]
  // in two roundings.  (Behind the fields above: the kernel arguments of the three planar formats stay where they were.)
  int swapRB; float nscale[3], nbias[3];
  // the 3-D LUT (vvr_set_output_lut3d, the definition: vvr.h), last before the store; lut == NULL: none.  lut: the device copy, one 8-byte node
  // R, G, B, 0 (16-bit words) at ( jb * lutN + jg ) * lutN + jr; lutN: 17, 33 or 65; lutShift: s = 16 - log2( lutN - 1 ).  Its input is Ek under a
  // transform, else the value of the matrix above at od = bd widened to 16 bits: ( v * 65535 + ( M >> 1 ) ) / M, M = 2^bd - 1 = maxOut - which
  // the kernel takes as ( x * lutWiden ) >> 39 with lutWiden = 2^39 / M + 1 (exact for x < 2^26: the error x / 2^39 stays below 1 / M)
  const uint16_t* lut; int lutN, lutShift; uint32_t lutWiden;
};
// ... and the regions of a batch for k_output_rgb (blockIdx.z): region z reads plane c at p.src[c] + srcOff[3 * z + c] (the table of PlaneRegions;
// NULL: none) + z * srcStep[c] samples (the resampled frames of the regions, back to back) and stores plane c at its place + z * dstStep[c] bytes.
struct RgbRegions
{
  int count = 1;
  const uint32_t* srcOff = nullptr;
  size_t srcStep[3] = { 0, 0, 0 }, dstStep[3] = { 0, 0, 0 };
};
void launch_output_rgb( hipStream_t s, const OutputRgbParams& p, void* dst, const RgbRegions& rg = RgbRegions() );
// a frame of the output queue as Y'CbCr at 4:4:4 or 4:2:2 (VVR_OUT_YUV444P8 ... VVR_OUT_Y410, the definition: vvr.h): one 4:2:0 frame of w x h luma
// samples (even), the luma as it is, the chroma brought to the luma grid as launch_output_rgb brings it there (4:4:4: bits 0 and 1 of collocated)
// or to every luma row of its own columns (4:2:2: the vertical 4-tap alone, bit 1 of collocated).  Three planes or one leave, rows back to back,
// into dst + dstOff[c] (256-byte aligned) or direct[c] (32-byte aligned memory of the caller's); nothing behind a plane's last row is written
// (a V210 row is ( ( w + 5 ) / 6 ) * 16 bytes, stored whole).  shift: the widening of the sample - 16 - bd (Y210), 10 - bd (V210, Y410), else 0.
struct OutputYuvParams
{
  const pel_t* src[3]; int stride[3], w, h; size_t dstOff[3];
  uint8_t* direct[3];
  int format, collocated, maxVal, shift;
  // the four byte formats in a context of 9 or 10 bits: the reduction at the store (narrow.s != 0; the kernel's NARROW variants).  (Behind the
  // fields above: the kernel arguments of the instantiations that serve every other request stay where they were.)
  NarrowArgs narrow;
};
void launch_output_yuv( hipStream_t s, const OutputYuvParams& p, void* dst );
// light-level statistics of the output queue (vvr_stats_submit, the definition: vvr.h).  launch_output_stats: the window src / stride / w / h of p
// (rgb != 0: the 4:2:0 frame with collocated and the matrix at od = bd, as launch_output_rgb takes it; else src[0] alone) accumulated into
// `shards`: STATS_SHARDS copies of STATS_WORDS words, all zero before the launch - hist_y[1024], hist_maxrgb[1024], max_c[3], then maxVal - min_c[3]
// (a maximum too, so that zero is the start of every word).  A workgroup adds into the copy its index selects: the workgroups of a flat frame all
// add to one bin, and adds to one address take their turn at the memory side.  launch_output_stats_sum: out[i] = the sum (the last six words: the
// maximum) over the copies.
#define STATS_SHARDS 16
#define STATS_WORDS 2054
#define RGB_FMT_STATS 255      /* the store class of k_output_rgb that accumulates where the others store */
void launch_output_stats( hipStream_t s, const OutputRgbParams& p, int rgb, uint32_t* shards );
void launch_output_stats_sum( hipStream_t s, const uint32_t* shards, uint32_t* out );
// a picture compared with a reference frame (vvr_compare_submit, the definition: vvr.h).  The window is cut into blocks of 64 x 64 luma samples
// (with them the 32 x 32 chroma samples of each chroma component), nbx x nby of them, row-major.  launch_output_compare: recs[( c * nbx * nby + b ) *
// CMP_REC_WORDS ..] = the record of component c in block b - sse (low word, high word), sad, the number of differing samples, the largest |d|, the
// smallest j * w[c] + i of a differing sample ( i, j ) of the component's window (0xffffffff: none) - and map[b] = the differing samples of the
// block over the components; every word is stored, nothing has to be cleared.  launch_output_compare_sum: out[c * CMP_OUT_WORDS ..] = sse, sad and
// the count as 64-bit sums (low word first), the maximum, the minimum of the first indices, over the blocks.
#define CMP_REC_WORDS 6
#define CMP_OUT_WORDS 8
struct CompareParams
{
  const pel_t* src[3]; int stride[3];            // the window's origin in the slot's planes; samples
  const uint8_t* ref[3]; size_t refStride[3];    // the reference window; bytes
  int w[3], h[3];                                // the window per component
  int numComp, refBytes, nbx, nby;               // refBytes: 1 or 2 per reference sample
  int bySample;                                  // no wide loads: an origin, a base or a stride does not allow them (chosen by the caller)
};
void launch_output_compare( hipStream_t s, const CompareParams& p, uint32_t* recs, uint32_t* map );
void launch_output_compare_sum( hipStream_t s, const uint32_t* recs, int blocks, int numComp, uint32_t* out );
// ... of a window rescaled on the way (vvr_set_compare_scaling, the definition: vvr.h): k_rescale's tile with the comparison where the store was -
// the rescaled sample never reaches memory.  rs[c]: the rescaling of component c as launch_rescale takes it (bytesPerSample is not looked at);
// ref / refStride / refBytes / nbx / nby: as CompareParams, of the RESCALED window; byByte: 2-byte reference samples are read as two bytes (an odd
// base or stride).  One launch for all components: workgroup g takes tile g - first[c] of component c, first[c] <= g < first[c + 1], tilesX[c]
// tiles of RS_TW = 64 columns a row, tileH[c] output rows each - a power of two, at most 64 for luma and 32 for chroma, so that a tile lies in one
// row of blocks; a luma tile lies in one block, a chroma tile in two, a half each.  The tiles of a block meet in its record through integer
// atomics - 64-bit add, 32-bit add, max, min: the result does not depend on their order - so the launcher first puts every record into the state
// "nothing differs" (0, 0, 0, 0, 0, 0xffffffff) and every map word to 0: clearWords words in all.  The records and the map are then what
// launch_output_compare leaves for the rescaled planes, word for word.
struct CompareScaledParams
{
  RescaleParams rs[3];
  const uint8_t* ref[3]; size_t refStride[3];
  int numComp, refBytes, nbx, nby, byByte;
  int tileH[3], rowsCap[3], tilesX[3], first[4];      // (set by compare_scaled_geometry)
};
struct CompareScaledGeometry { size_t ldsBytes, clearWords; };
// the tile height of launch_rescale brought down to a power of two: the source rows of a tile fit RS_ROWS rows of sums; 64- and 32-row tiles only
// where the component still has about a thousand of them
inline CompareScaledGeometry compare_scaled_geometry( CompareScaledParams& p )
{
  CompareScaledGeometry g = { 0, (size_t) ( CMP_REC_WORDS * p.numComp + 1 ) * p.nbx * p.nby };
  p.first[0] = 0;
  for( int c = 0; c < 3; c++ )
  {
    p.tileH[c] = p.rowsCap[c] = p.tilesX[c] = 0; p.first[c + 1] = p.first[c];
    if( c >= p.numComp ) continue;
    const RescaleParams& r = p.rs[c];
    const int taps = r.luma ? 8 : 4, fracShift = r.luma ? 4 : 5;
    auto rows = [&]( int t ) { const int64_t den = (int64_t) 1 << ( r.shiftY + fracShift ); return (int) ( ( (int64_t) ( t - 1 ) * r.stepY + den - 1 ) / den ) + taps; };
    int tileH = c ? 32 : 64;
    while( tileH > 1 && rows( tileH ) > 128 /* RS_ROWS */ ) tileH >>= 1;
    const int tilesX = ( r.outW + 63 ) / 64;
    while( tileH > 16 && (int64_t) tilesX * ( ( r.outH + tileH - 1 ) / tileH ) < 1000 ) tileH >>= 1;
    p.tileH[c] = tileH; p.tilesX[c] = tilesX; p.rowsCap[c] = rows( tileH ) < r.h ? rows( tileH ) : r.h;
    p.first[c + 1] = p.first[c] + tilesX * ( ( r.outH + tileH - 1 ) / tileH );
    const size_t lds = (size_t) p.rowsCap[c] * 64 * sizeof( int );
    if( lds > g.ldsBytes ) g.ldsBytes = lds;
  }
  return g;
}
void launch_output_compare_scaled( hipStream_t s, CompareScaledParams p, uint32_t* recs, uint32_t* map );
// SSIM of a picture against a reference frame (vvr_ssim_submit, the definition: vvr.h), on the comparison's parameters and blocks: a block owns the
// SSIM windows (8 x 8 samples at a stride of 4) whose ORIGIN lies in it.  launch_output_ssim: recs[( c * nbx * nby + b ) * SSIM_REC_WORDS ..] = the
// record of component c in block b - the sum of v (low word, high word), then the smallest v with the first window that has it as ONE 64-bit key,
// low word first: ( (uint32_t) v ^ 0x80000000 ) << 32 | gj * windows_x + gi for window ( gi, gj ) of the component's grid, so that the smaller key is
// the smaller v and, among equals, the earlier window in raster order; all ones: no window - and map[b] = the smallest v of the block over the
// components (0x7fffffff: none); every word is stored, nothing has to be cleared.  launch_output_ssim_sum: out[c * SSIM_OUT_WORDS ..] = the sum and
// the smallest key over the blocks, in the same four words.
#define SSIM_REC_WORDS 4
#define SSIM_OUT_WORDS 4
#define SSIM_NO_WINDOW 0xffffffffffffffffull
void launch_output_ssim( hipStream_t s, const CompareParams& p, int bitDepth, uint32_t* recs, int32_t* map );
void launch_output_ssim_sum( hipStream_t s, const uint32_t* recs, int blocks, int numComp, uint32_t* out );
// MS-SSIM of a picture against a reference frame (vvr_msssim_submit, the definition: vvr.h): a launch per level on the SSIM request's blocks, then
// one fold.  launch_output_msssim: p describes ONE level - level 0 as launch_output_ssim takes it, a deeper level with src and ref pointing to the
// level's two scratch planes (16-bit words, refBytes 2, rows a multiple of 16 bytes: the wide class) - and recs[( c * nbx * nby + b ) *
// MSSSIM_REC_WORDS ..] = the record of component c in block b: the sum of c, the contrast-structure quotient, then the sum of v, both 64 bits, low
// word first; every word is stored, nothing has to be cleared.  next != NULL: the launch also writes level k + 1 of both images, the 2 x 2 rounded
// means of the clamped samples, into next->x[c] (the slot's side) and next->y[c] (the reference's), rows of next->stride[c] samples (a multiple of
// 8, the bases at a multiple of 16 bytes) - from the whole 4 x 4 cells of level k only: sample ( i, j ) of level k + 1 is written for
// i < 2 * ( w_k / 4 ) and j < 2 * ( h_k / 4 ), which is all a window of level k + 1 or deeper reads.  launch_output_msssim_sum: a launch for all
// levels, out[( k * numComp + c ) * MSSSIM_OUT_WORDS ..] = the two sums over the blocks[k] blocks of level k, whose records start at recs + recOff[k].
#define MSSSIM_REC_WORDS 4
#define MSSSIM_OUT_WORDS 4
#define MSSSIM_MAX_SCALES 5
struct MsssimNext { uint16_t* x[3]; uint16_t* y[3]; int stride[3]; };
struct MsssimFold { int scales, recOff[MSSSIM_MAX_SCALES], blocks[MSSSIM_MAX_SCALES]; };      // recOff: in words, a multiple of 64
void launch_output_msssim( hipStream_t s, const CompareParams& p, int bitDepth, uint32_t* recs, const MsssimNext* next );
void launch_output_msssim_sum( hipStream_t s, const uint32_t* recs, const MsssimFold& f, int numComp, uint32_t* out );
// XPSNR of a picture against a reference frame (vvr_xpsnr_submit, the definition: vvr.h), on the comparison's parameters and tiles of 64 x 64 luma
// samples (p.nbx x p.nby of them), one launch.  recs: blocksX * blocksY records of XPSNR_REC_WORDS 64-bit words, row-major, laid out as a
// vvr_xpsnr_block - sse of the three components, the sum of |f|, the sum of t, then count in the low half of the last word - which the caller has
// CLEARED: the launch adds to them (integer adds, exact in any order).  block: B, a multiple of 4; filter: 1 or 2; temporal: 0 .. 2 with
// prev[0 .. temporal - 1], luma planes of the window's size, prevStride in bytes, p.refBytes per sample; p.bySample also stands for their bases
// and strides.
#define XPSNR_REC_WORDS 6
struct XpsnrParams { CompareParams c; const uint8_t* prev[2]; size_t prevStride[2]; int block, blocksX, blocksY, filter, temporal; };
void launch_output_xpsnr( hipStream_t s, const XpsnrParams& p, unsigned long long* recs );
// decoded picture hash of the output queue (vvr_hash_submit): CRC (crc != 0) or checksum of every component of a picture, finished on the device.
// launch_hash_rows: one launch over the rows of all planes, rows[g] = the CRC piece (the row's bytes mod P, register from 0) or the checksum share
// of row g (the planes' rows one after the other).  launch_hash_combine: out[c] = the component's digest as a number - the checksum, or the CRC
// register after chaining the rows from 0xffff and the 16 appended zero bits.  The powers of x (mod P) the kernels multiply by come from the
// host (vvr_output.inc, hash_params): bits = 8 or 16 per sample, a lane folds chunks of 8 samples
struct HashParams
{
  const pel_t* src[3]; int stride[3], w[3], h[3];
  int numComp, two, crc;
  uint32_t xIter, xTree[6], xTail[3];            // rows: x^( 64 chunks ); x^( chunk << s ); x^( ( w[c] & 7 ) * bits )
  uint32_t xRowIter[3], xRowTree[3][7];          // combine: x^( 256 rows of component c ); x^( row << s )
};
void launch_hash_rows( hipStream_t s, const HashParams& p, uint32_t* rows );
void launch_hash_combine( hipStream_t s, const HashParams& p, const uint32_t* rows, uint32_t* out );
void launch_mc_affine( hipStream_t s, const PicDev& pic, const RefSet& refs, DevPlanes reco, const McItem* items, int numItems );
void launch_mc_rpr( hipStream_t s, const PicDev& pic, const RefSet& refs, DevPlanes reco, const McItem* items, int numItems );      // tiles of CUs with a scaled reference picture
void launch_mc_dmvr( hipStream_t s, const PicDev& pic, const RefSet& refs, DevPlanes reco, const McItem* items, int numItems, int32_t* dmvrOut );
void launch_intra  ( hipStream_t s, const PicDev& pic, DevPlanes reco, DevPlanes resi, const IntraItem* items, int numItems, const IntraUnit* units, int numUnits, int ticket0, int ticket1, int numWorkgroups, int* sync, int wide,
                     uint32_t* maps = nullptr, size_t mapInts = 0, int mapW4 = 0, int mapH4 = 0, int* errWord = nullptr );      // maps (a picture whose units are all whole CTUs of intra CUs): the per-cell words - the CTU wavefront is resolved block by block (k_intra<.., FINE>)      // the units [ticket0, ticket1); wide: an I picture the stream waits for (eight wavefronts per workgroup)
void launch_resi_add( hipStream_t s, const PicDev& pic, DevPlanes reco, DevPlanes resi, const IntraItem* items, int numItems );      // scaled chroma residuals of inter blocks (between the luma and the chroma units)
size_t intra_sync_ints( int numUnits, int numItems );      // ints `sync` has to hold: ticket, unit flags, the blocks' parameter records
// the intra stage of a picture with scattered intra blocks (vvr_intra_leaf.inc): one wavefront per block of `items` (decoding order per component), ordered through
// per-cell words in `maps` (intra_leaf_map_ints words for the largest picture of the context: all zero between launches)
#define IT_MODE_CSFAC 253      /* mode value: the LMCS chroma scaling factor of VPDU IntraItem::tu (no samples) */
size_t intra_leaf_map_ints( int w4, int h4, int vpdus );
// The picture's first launch (k_prep): the passes over its records that depend on nothing but the uploaded image - the motion-compensation tiles of the CUs
// the host only counted, the cell maps of the deblocking edge derivation (lfMaps), the cells and the ticket of the scattered intra blocks (numItems)
struct PrepWork
{
  const McCuRef* mcCus = nullptr; int numMcCus = 0; McItem *plain = nullptr, *bdof = nullptr, *dmvr = nullptr;
  bool lfMaps = false; uint32_t numCu = 0, numTu = 0; struct LfCell *cell = nullptr, *cellC = nullptr; struct LfMv* mv = nullptr; uint32_t* ref = nullptr; const struct LfSbCell* sb = nullptr; int numSb = 0;
  const IntraItem *items = nullptr, *resi = nullptr; int numItems = 0, numResi = 0; uint32_t* maps = nullptr; size_t mapInts = 0; int mapW4 = 0, mapH4 = 0;
  const TbItem* tbItems[3] = { nullptr, nullptr, nullptr }; TbRec* tbRecs[3] = { nullptr, nullptr, nullptr }; int numTb[3] = { 0, 0, 0 };      // the transform blocks' records (prep_tb_records)
};
void launch_prep( hipStream_t s, const PicDev& pic, const PrepWork& w );
void launch_intra_leaf( hipStream_t s, const PicDev& pic, DevPlanes reco, DevPlanes resi, const IntraItem* items, int numItems, const IntraItem* resiItems, int numResi /* residual-add blocks grouped by VPDU: done by the VPDU's IT_MODE_CSFAC item */,
                        uint32_t* maps, size_t mapInts, int mapW4, int mapH4, int* errWord /* the job's error word: pinned host memory the device writes when a bounded wait gave up */ );

