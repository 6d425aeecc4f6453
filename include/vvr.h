/*
 * vvr.h — C ABI of the MI355X-native VVC reconstruction back-end ("vvr" = VVC reconstruction).
 *
 * This is the drop-in boundary for the reconstruction stage of VVdeC.  It replaces the inner seam
 *     DecLibRecon::create / destroy / decompressPicture / waitForPrevDecompressedPic / getCurrPic
 *     (reference: source/Lib/DecoderLib/DecLibRecon.h:143-200, called only from DecLib::reconPicture and
 *      DecLib::blockAndFinishPictures, source/Lib/DecoderLib/DecLib.cpp:612-655)
 * with plain-C entry points: plain pointers and sizes, status codes instead of exceptions, no C++/torch types.
 *
 * Contract on entry of vvr_submit (mirrors the contract on entry of decompressPicture):
 *   - the host parser has produced, for one picture, the per-CTU / per-CU / per-TU mode records, the quantised
 *     coefficient levels (reference: written by CABACReader.cpp:2457-2478 into the reco plane; here: a packed
 *     int16 stream, only the [0..maxScanPosX] x [0..maxScanPosY] corner of every coded transform block),
 *     the final motion field after MV derivation ("MIDER", DecCu.cpp:62/720 — stays on the host), and the
 *     deblocking edge parameters (LoopFilter::calcFilterStrengthsCTU, LoopFilter.cpp:360/495 — stays on the host);
 *   - reference pictures are identified by DPB slot numbers owned by this context.
 * Contract on exit of vvr_wait: the three planes of the output slot hold the final (post deblock/SAO/ALF) samples,
 *   identical to the reference decoder's output for the same records (VVC is an integer specification).
 *
 * All structs are little-endian PODs with fixed layout; arrays are struct-of-arrays per picture.
 * Coordinates are in LUMA samples unless a field says otherwise.  Only 4:2:0 and 4:0:0 are accepted in this version.
 */
#ifndef VVR_H
#define VVR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define VVR_API __attribute__((visibility("default")))
#else
#define VVR_API
#endif

#define VVR_ABI_VERSION 5

/* ------------------------------------------------------------------------------------------------------------------
 * status codes (negative = error; mirrors the style of vvdecErrorCodes, include/vvdec/vvdec.h.in:91-105)
 * ---------------------------------------------------------------------------------------------------------------- */
enum {
  VVR_OK               = 0,
  VVR_ERR_UNSPECIFIED  = -1,
  VVR_ERR_PARAMETER    = -2,   /* inconsistent picture description                                  */
  VVR_ERR_UNSUPPORTED  = -3,   /* a coding tool / format this build does not reconstruct            */
  VVR_ERR_DEVICE       = -4,   /* HIP runtime error (message via vvr_last_error)                    */
  VVR_ERR_NO_DEVICE    = -5,   /* no usable gfx950 device: the back-end never falls back to the CPU */
  VVR_NOT_READY        = 1,    /* (non-blocking queries) the pictures concerned have not been handed to the device yet: ask again */
  VVR_ERR_BUSY         = -6,   /* DPB slot still in use / too many pictures in flight               */
};

/* ------------------------------------------------------------------------------------------------------------------
 * picture-level description
 * ---------------------------------------------------------------------------------------------------------------- */
#define VVR_MAX_REFS      16
#define VVR_MAX_ALF_APS    8
#define VVR_ALF_CLASSES   25
#define VVR_ALF_LUMA_TAPS 13   /* 12 symmetric taps + centre (centre entry unused)   */
#define VVR_ALF_CHR_TAPS   7   /*  6 symmetric taps + centre                         */
#define VVR_ALF_MAX_CHR_ALT 8
#define VVR_CCALF_FILTERS  4
#define VVR_CCALF_TAPS     7   /* MAX_NUM_CC_ALF_CHROMA_COEFF - 1 signalled taps + pad */

/* tool_flags */
enum {
  VVR_TOOL_SAO_LUMA     = 1u << 0,   /* slice_sao_luma_flag                                        */
  VVR_TOOL_SAO_CHROMA   = 1u << 1,
  VVR_TOOL_ALF          = 1u << 2,   /* sps ALF on and at least one component enabled in the slice */
  VVR_TOOL_CCALF        = 1u << 3,
  VVR_TOOL_LMCS         = 1u << 4,   /* slice LMCS enabled (luma mapping)                          */
  VVR_TOOL_LMCS_CSCALE  = 1u << 5,   /* chroma residual scaling                                    */
  VVR_TOOL_DEBLOCK_OFF  = 1u << 6,   /* deblocking disabled for the picture                        */
  VVR_TOOL_DEP_QUANT    = 1u << 7,
  VVR_TOOL_BDOF         = 1u << 8,   /* sps BDOF on and not disabled in the picture header         */
  VVR_TOOL_DMVR         = 1u << 9,
  VVR_TOOL_PROF         = 1u << 10,
  VVR_TOOL_JCCR_SIGN    = 1u << 11,  /* ph_joint_cbcr_sign_flag                                    */
  VVR_TOOL_STILL_REF    = 1u << 12,  /* picture is still referenced: DMVR refined MVs are returned */
  VVR_TOOL_LFNST        = 1u << 13,  /* sps LFNST on (TrQuant.cpp:301)                              */
  VVR_TOOL_MTS          = 1u << 14,  /* sps MTS on (explicit+implicit selection resolved per TU)    */
  VVR_TOOL_CCLM_COLLOC  = 1u << 15,  /* sps_chroma_vertical_collocated_flag: CCLM down-samples luma with the 5-tap cross filter */
  VVR_TOOL_WP           = 1u << 16,  /* explicit weighted prediction applies to this picture: P slice with pps_weighted_pred_flag or
                                        B slice with pps_weighted_bipred_flag (InterPrediction.cpp:707,735-742); vvr_picture.wp set */
  VVR_TOOL_SCALING_LIST = 1u << 17,  /* explicit scaling list in use for the slice (Quant.cpp:330-336); vvr_picture.scaling set */
  VVR_TOOL_SCALING_LIST_NO_LFNST = 1u << 18,  /* sps_scaling_matrix_for_lfnst_disabled_flag */
  VVR_TOOL_IMPLICIT_MTS = 1u << 19,  /* MTS on without sps_explicit_mts_intra_enabled_flag: intra luma blocks use the implicit DST-7 rule.
                                        Informative (vvr_tu.tr_type is already resolved); a checker that drives the reference decoder needs it */
  VVR_TOOL_IBC          = 1u << 20,  /* sps_ibc_enabled_flag: the picture may hold VVR_PRED_IBC CUs (InterPrediction::xIntraBlockCopy,
                                        InterPrediction.cpp:1995).  Block vector in vvr_cu.mv[0][0] (1/16 units, integer sample
                                        positions); it must point at samples of the same CTU row that precede the CU in decoding order
                                        and still sit in the IBC virtual buffer (CodingStructure::fillIBCbuffer, CodingStructure.cpp:550) */
  VVR_TOOL_LADF         = 1u << 21,  /* sps_ladf_enabled_flag: luma-adaptive deblocking, parameters in vvr_pic_header.ladf_* (LoopFilter.cpp:1363,1519).
                                        Informative like VVR_TOOL_IMPLICIT_MTS: the back-end looks at ladf_num_intervals                       */
  VVR_TOOL_NO_LF_ACROSS_SLICES = 1u << 22,  /* !pps_loop_filter_across_slices_enabled_flag: SAO and ALF do not look across slice boundaries (the deblocking
                                        edges there are already switched off in the edge-parameter table the host derives)                     */
  VVR_TOOL_NO_LF_ACROSS_TILES  = 1u << 23,  /* !pps_loop_filter_across_tiles_enabled_flag, likewise for tile boundaries                              */
  VVR_TOOL_AFFINE_MV_ON_DEVICE = 1u << 24,  /* the sub-block MVs of affine CUs are spanned by the back-end from the CU's control-point MVs (cu.mv[list][0..2];
                                               PU::setAllAffineMv, UnitTools.cpp:2689): vvr_picture.motion is not read for affine CUs and need not hold them   */
  VVR_TOOL_COL_MOTION   = 1u << 25,  /* the back-end keeps the picture's collocated motion (the TMVP storage of later pictures): vvr_picture.motion at every
                                        second 4x4 unit in both directions, with the MVs of DMVR CUs replaced by the refined ones as soon as the DMVR
                                        kernel has them (DecCu::TaskFinishMotionInfo, DecCu.cpp:161-253).  vvr_read_col_motion() hands it out; the host
                                        neither reads the delta MVs nor patches / subsamples its motion field                                      */
  VVR_TOOL_LFP_ON_DEVICE = 1u << 26, /* the back-end derives the deblocking edge parameters itself (the reference's LF_INIT task, LoopFilter::
                                        calcFilterStrengthsCTU, LoopFilter.cpp:495-1360) from the CU / TU records: vvr_picture.lfp is not read and may be NULL.
                                        vvr_picture.motion then has to hold the cells of SbTMVP and GPM CUs - and of affine CUs unless
                                        VVR_TOOL_AFFINE_MV_ON_DEVICE is set - (the motion of every other CU is in its record); a slice that switches
                                        deblocking off in a picture that deblocks says so with VVR_TOOL_DEBLOCK_OFF in its vvr_slice_header.tool_flags       */
};

typedef struct vvr_alf_params {     /* final filters, AdaptiveLoopFilter::reconstructCoeff (AdaptiveLoopFilter.cpp:888) stays on the host */
  int16_t luma_coeff[VVR_MAX_ALF_APS][VVR_ALF_CLASSES][VVR_ALF_LUMA_TAPS];   /* un-transposed, per class                 */
  int16_t luma_clip [VVR_MAX_ALF_APS][VVR_ALF_CLASSES][VVR_ALF_LUMA_TAPS];   /* clipping VALUES (m_alfClippVls resolved)  */
  int16_t chroma_coeff[VVR_ALF_MAX_CHR_ALT][VVR_ALF_CHR_TAPS];               /* per alternative (shared by Cb and Cr)     */
  int16_t chroma_clip [VVR_ALF_MAX_CHR_ALT][VVR_ALF_CHR_TAPS];
  int16_t ccalf_coeff[2][VVR_CCALF_FILTERS][VVR_CCALF_TAPS + 1];
  uint8_t num_luma_aps;             /* alfCtbFilterIndex >= 16 selects luma_coeff[idx-16]                                  */
  uint8_t pad[7];
} vvr_alf_params;

typedef struct vvr_lmcs_params {    /* Reshape::constructReshaper (Reshape.cpp:318) stays on the host */
  int16_t fwd_lut[1024 * 4];        /* forward map of every sample value (rspFwdCore, Buffer.cpp:321), 1 << bit_depth entries used */
  int16_t inv_lut[1024 * 4];        /* inverse map (m_invLUT)                                                                      */
  int16_t chroma_scale[16];         /* m_chromaAdjHelpLUT                                                                          */
  int16_t pivot[17];                /* m_reshapePivot                                                                              */
  int16_t min_bin, max_bin;         /* lmcs_min_bin_idx, LmcsMaxBinIdx (Reshape::getPWLIdxInv, :280)                               */
  /* the syntax-level model the tables were built from (lmcs_data()): the back-end does not read it; it lets a checker that
   * drives the reference decoder's own Reshape class rebuild the same tables */
  int16_t model_delta_cw[16];       /* lmcsDeltaCW[i] (signed)  */
  int16_t model_delta_crs;          /* lmcsDeltaCrs             */
  int16_t pad[4];
} vvr_lmcs_params;

typedef struct vvr_wp_entry {        /* WPScalingParam (Slice.h:2215) of one reference picture and component, as parsed */
  int16_t weight;                    /* iWeight ( 1 << log2_denom when the flag is off )                       */
  int16_t offset;                    /* iOffset, in 8-bit units (scaled by 1 << (bit_depth - 8) when applied)  */
  uint8_t present;                   /* bPresentFlag (luma_weight_lX_flag / chroma_weight_lX_flag)             */
  uint8_t pad[3];
} vvr_wp_entry;

typedef struct vvr_wp_params {       /* pred_weight_table(): Slice::m_weightPredTable (Slice.h:2560) */
  uint8_t      log2_denom[2];        /* uiLog2WeightDenom of luma / chroma                           */
  uint8_t      pad[6];
  vvr_wp_entry e[2][VVR_MAX_REFS][3];/* [list][refIdx][Y, Cb, Cr]                                    */
} vvr_wp_params;

typedef struct vvr_scaling_list {    /* ScalingList after scaling_list_data() decoding (prediction / DPCM resolved) */
  uint8_t coef[28][64];              /* m_scalingListCoef[id]: ids 0-1 are 2x2 (4 entries), 2-7 4x4 (16), 8-27 8x8 (64), raster order */
  uint8_t dc[28];                    /* m_scalingListDC[id] (ids >= 14: the DC of the up-sampled 16x16 .. 64x64 matrices) */
  uint8_t pad[4];
} vvr_scaling_list;

typedef struct vvr_pic_header {
  uint32_t abi_version;             /* VVR_ABI_VERSION                                                  */
  uint32_t tool_flags;              /* VVR_TOOL_*                                                       */
  uint16_t width, height;           /* luma samples                                                     */
  uint8_t  chroma_format;           /* 0 = 4:0:0, 1 = 4:2:0                                             */
  uint8_t  bit_depth;               /* 8..10 (Main 10)                                                  */
  uint8_t  log2_ctu;                /* 5..7                                                             */
  uint8_t  slice_type;              /* 0 B, 1 P, 2 I  (SliceType, CommonDef.h)                          */
  int32_t  poc;
  int16_t  out_slot;                /* DPB slot that receives the reconstruction                        */
  int8_t   num_ref[2];
  int16_t  ref_slot[2][VVR_MAX_REFS];
  int32_t  ref_poc [2][VVR_MAX_REFS];
  int8_t   deblock_beta_offset_div2[3];   /* Y, Cb, Cr (LoopFilter.cpp:1473,1637)                       */
  int8_t   deblock_tc_offset_div2[3];
  uint8_t  log2_sao_offset_scale[2];      /* luma, chroma                                               */
  int8_t   min_qp_ts;               /* 4 + 6*internalMinusInputBitDepth (Quant.cpp:104)                  */
  uint8_t  ladf_num_intervals;      /* 0: LADF off; else sps_num_ladf_intervals_minus2 + 2 (2..5), LoopFilter::deriveLADFShift (LoopFilter.cpp:1363) */
  int8_t   ladf_qp_offset[5];       /* SPS::getLadfQpOffset(k): [0] = sps_ladf_lowest_interval_qp_offset   */
  uint8_t  pad;
  int16_t  ladf_lower_bound[5];     /* SPS::getLadfIntervalLowerBound(k), luma level; [0] unused           */
  /* virtual boundaries of the picture header (ph_virtual_boundaries_present_flag; PicHeader::getVirtualBoundariesPosX / PosY, Slice.h): luma
   * positions, multiples of 8, inside the picture, ascending.  The in-loop filters do not work across them: edges on a boundary are not
   * deblocked (that is part of the edge tables the host supplies, LoopFilter.cpp:669-690), SAO leaves the two sample columns / rows at a
   * boundary alone for the edge classes that look across it (SampleAdaptiveOffset.cpp:823), ALF filters every part of a CTU the boundaries cut
   * out with its own replicated border (AdaptiveLoopFilter.cpp:142-175,764-850).                                                              */
  uint8_t  num_ver_vb, num_hor_vb;  /* 0..3 each                                                          */
  uint16_t wrap_offset;             /* 0: off; else pps_ref_wraparound_enabled_flag with PPS::getWrapAroundOffset() luma samples: motion compensation reads
                                       a reference picture as if it wrapped around horizontally at that period (360-degree video; wrapClipMv, Mv.cpp:112,
                                       Picture::extendPicBorderWrap, Picture.cpp:410).  Multiple of 8, CTU size + 16 .. picture width                        */
  uint8_t  pad2[2];
  uint16_t vb_pos_x[3], vb_pos_y[3];
  uint8_t  pad3[4];
} vvr_pic_header;

/* ------------------------------------------------------------------------------------------------------------------
 * coding unit  (source of each field: CodingUnit, source/Lib/CommonLib/Unit.h:314-420)
 * ---------------------------------------------------------------------------------------------------------------- */
enum { VVR_PRED_INTER = 0, VVR_PRED_INTRA = 1, VVR_PRED_IBC = 2 };
enum { VVR_TREE_JOINT = 0, VVR_TREE_LUMA = 1, VVR_TREE_CHROMA = 2 };   /* which components the CU carries */

/* cu.flags */
enum {
  VVR_CU_ROOT_CBF   = 1u << 0,
  VVR_CU_SKIP       = 1u << 1,
  VVR_CU_MERGE      = 1u << 2,
  VVR_CU_AFFINE     = 1u << 3,
  VVR_CU_AFFINE_6P  = 1u << 4,
  VVR_CU_CIIP       = 1u << 5,
  VVR_CU_GEO        = 1u << 6,
  VVR_CU_SBTMVP     = 1u << 7,   /* mergeType == MRG_TYPE_SUBPU_ATMVP                                       */
  VVR_CU_MIP        = 1u << 8,
  VVR_CU_MIP_TRANSP = 1u << 9,
  VVR_CU_SMVD       = 1u << 10,
  VVR_CU_MMVD       = 1u << 11,
};

/* cu.mc_mode: the branch InterPrediction::motionCompensation (InterPrediction.cpp:1372-1459) takes for this CU.
 * Resolving it needs POCs/flags only and is done once per CU by the host glue (integration/vvr_extract.h::resolveMcMode). */
enum {
  VVR_MC_NONE = 0,
  VVR_MC_UNI,          /* one list, or identical-motion shortcut (xCheckIdenticalMotion, :404)          */
  VVR_MC_BI,           /* xPredInterBi: two lists + addAvg / BCW                                        */
  VVR_MC_BDOF,         /* xSubPuBio (:551)                                                              */
  VVR_MC_DMVR,         /* xProcessDMVR (:1847), BDOF decided per sub-block                              */
  VVR_MC_DMVR_BDOF,
  VVR_MC_AFFINE,       /* xPredAffineBlk (:934) (+PROF)                                                 */
  VVR_MC_SBTMVP,       /* xSubPuMC (:438)                                                               */
  VVR_MC_GEO,          /* motionCompensationGeo (:1461)                                                 */
};

typedef struct vvr_cu {
  uint16_t x, y;                 /* luma position                                                            */
  uint8_t  w, h;                 /* luma size (chroma-tree CU: luma-equivalent area)                         */
  uint8_t  tree;                 /* VVR_TREE_*                                                               */
  uint8_t  pred_mode;            /* VVR_PRED_*                                                               */
  uint16_t flags;                /* VVR_CU_*                                                                 */
  int8_t   qp;                   /* cu.qp (luma QP without QpBdOffset)                                       */
  uint8_t  mc_mode;              /* VVR_MC_*                                                                 */
  /* intra */
  uint8_t  intra_dir[2];         /* FINAL modes (PU::getFinalIntraMode, UnitTools.cpp:587): 0 planar, 1 DC, 2..66, 67..69 LM/MDLM_L/MDLM_T; MIP: mode id */
  uint8_t  multi_ref_idx;        /* 0..2                                                                     */
  uint8_t  isp_mode;             /* 0 none, 1 HOR_INTRA_SUBPARTITIONS, 2 VER                                  */
  uint8_t  bdpcm[2];             /* luma, chroma: 0 off, 1 hor, 2 ver                                        */
  uint8_t  lfnst_idx;            /* 0..2                                                                     */
  uint8_t  sbt_info;             /* CodingUnit::_sbtInfo                                                     */
  /* inter */
  uint8_t  inter_dir;            /* 1 L0, 2 L1, 3 bi                                                         */
  int8_t   ref_idx[2];           /* -1 = unused                                                              */
  uint8_t  bcw_idx;              /* 0..4, BCW_DEFAULT = 2                                                    */
  uint8_t  imv;                  /* 3 = IMV_HPEL selects the alternative half-pel filter                     */
  uint8_t  geo_split_dir;
  uint8_t  geo_dir_ref[2];       /* interDirrefIdxGeo0/1: [i] = (interDir << 4) | refIdx, interDir 1 = L0, 2 = L1 */
  uint8_t  ciip_neigh_intra;     /* bit0: above neighbour intra, bit1: left neighbour intra (IntraPrediction.cpp:917-927) */
  uint8_t  lfnst_intra_mode;     /* intra mode used for LFNST set selection before wide-angle remap (TrQuant.cpp:213-221) */
  uint8_t  pad0[2];
  int32_t  mv[2][3][2];          /* [list][cpmv idx][hor,ver], 1/16 luma sample; [l][0] for translational     */
  int32_t  geo_mv[2][2];         /* GPM: the two uni-prediction MVs                                           */
  uint32_t first_tu, num_tu;     /* range in the TU array (decode order)                                     */
  uint32_t dmvr_off;             /* first entry of this CU in the DMVR delta-MV output array                 */
  uint32_t pad1;
} vvr_cu;

/* ------------------------------------------------------------------------------------------------------------------
 * transform unit  (TransformUnit, Unit.h:285-304)
 * ---------------------------------------------------------------------------------------------------------------- */
enum { VVR_MTS_DCT2 = 0, VVR_MTS_SKIP = 1, VVR_MTS_DST7_DST7 = 2, VVR_MTS_DCT8_DST7 = 3, VVR_MTS_DST7_DCT8 = 4, VVR_MTS_DCT8_DCT8 = 5 };

typedef struct vvr_tu {
  uint16_t x, y;                 /* luma position                                                            */
  uint8_t  w, h;                 /* luma size (chroma block = w/2 x h/2 for 4:2:0)                            */
  uint8_t  comp_mask;            /* bit c set: block of component c exists in this TU (dual tree / ISP)       */
  uint8_t  cbf;                  /* bit c: coded block flag of component c                                    */
  uint8_t  joint_cbcr;           /* 0 or jointCbCr mask (1,2,3)                                               */
  uint8_t  mts_idx[3];           /* VVR_MTS_* per component                                                   */
  uint8_t  max_scan_x[3];        /* last significant column per component (TransformUnit::maxScanPosX)       */
  uint8_t  max_scan_y[3];
  int8_t   qp[3];                /* QpParam::Qps[0] per component incl. QpBdOffset (Quant.cpp:65-101);        */
                                 /* for a joint-CbCr TU qp[1]/qp[2] hold the joint QP where ICT mode == 2     */
  uint8_t  tr_type[3];           /* (trTypeVer << 2) | trTypeHor with 0 DCT2, 1 DCT8, 2 DST7                   */
                                 /* = TrQuant::getTrTypes (TrQuant.cpp:330-407), resolved by the host glue     */
  uint8_t  pad0;
  uint32_t coef_off[3];          /* offset (int16 units) of this block's level corner in the coefficient stream */
  uint32_t cu;                   /* owning CU                                                                  */
} vvr_tu;

/* ------------------------------------------------------------------------------------------------------------------
 * per-4x4 side tables (picture raster order, stride = ceil(width/4))
 * ---------------------------------------------------------------------------------------------------------------- */
typedef struct vvr_motion {      /* MotionInfo, MotionInfo.h:122 */
  int32_t mv[2][2];              /* [list][hor,ver]                                                            */
  int8_t  ref_idx[2];            /* -1 unused (MI_NOT_VALID for intra; IBC: both -1, mv[0] = block vector, UnitTools.cpp:3018) */
  uint8_t pad[2];
} vvr_motion;

typedef struct vvr_lfp {         /* LoopFilterParam, TypeDef.h:694-707; semantics SURVEY.md Appendix D         */
  int8_t  qp[3];
  uint8_t bs;                    /* 2 bits per component                                                       */
  uint8_t side_max_filt_length;  /* [6:4] P, [2:0] Q, bit 7 transform edge                                     */
  uint8_t flags;                 /* bit0 filterEdge luma, bit1 filterEdge chroma, bit5 chroma large block      */
  uint8_t pad[2];
} vvr_lfp;

/* ------------------------------------------------------------------------------------------------------------------
 * per-CTU loop filter controls
 * ---------------------------------------------------------------------------------------------------------------- */
typedef struct vvr_sao_ctu {     /* SAOBlkParam after reconstructBlkSAOParam (merge resolved, offsets scaled)   */
  uint8_t mode[3];               /* 0 off, 1 on                                                                */
  uint8_t type[3];               /* 0 EO_0, 1 EO_90, 2 EO_135, 3 EO_45, 4 BO                                    */
  uint8_t band_pos[3];           /* BO: first band                                                             */
  int8_t  offset[3][4];          /* EO: classes {valley, half-valley, half-peak, peak}; BO: 4 consecutive bands */
  uint8_t pad[3];
} vvr_sao_ctu;

typedef struct vvr_alf_ctu {     /* CtuAlfData, CodingStructure.h:75 */
  uint8_t cc_idc[2];             /* 0 off, else filter index + 1                                               */
  uint8_t enable[3];
  uint8_t alt[2];                /* chroma alternative                                                         */
  uint8_t pad;
  int16_t luma_filter_idx;       /* < 16: fixed set, else APS idx - 16                                         */
  uint8_t pad2[2];
} vvr_alf_ctu;

typedef struct vvr_subpic {      /* SubPic (Slice.h:820): one sub-picture of the layout the SPS signals (sps_subpic_info_present_flag)        */
  uint16_t x0, y0, x1, y1;       /* luma samples, inclusive: getSubPicLeft / Top / Right / Bottom; x0, y0 on the CTU grid                      */
  uint8_t  treated_as_pic;       /* sps_subpic_treated_as_pic_flag: motion compensation of its CUs reads nothing outside the sub-picture       */
                                 /* (clipMvInSubpic, Mv.cpp:84; Picture::getSubPicBuf + DecLibRecon::createSubPicRefBufs, DecLibRecon.cpp:388)   */
  uint8_t  lf_across;            /* sps_loop_filter_across_subpic_enabled_flag: 0 = SAO and ALF of its CTUs do not look into other sub-pictures */
  uint8_t  pad[2];
} vvr_subpic;

/* ------------------------------------------------------------------------------------------------------------------
 * one picture to reconstruct
 * ---------------------------------------------------------------------------------------------------------------- */
/* What a slice header sets for its slice only (DecLibRecon switches on ctuData.slice per CTU, DecLibRecon.cpp:787-790,856-860; every stage reads
 * cu.slice / the CTU's slice: Quant.cpp:306,336, DecCu.cpp:383,460,489, LoopFilter.cpp:423,1473,1637, Reshape.cpp:385, AdaptiveLoopFilter.cpp:515,558,603).
 * NOT here, by construction of the description: the slice's reference picture lists - hdr.ref_slot / ref_poc hold the UNION of the slices' lists
 * per list (at most VVR_MAX_REFS pictures) and every cu.ref_idx / vvr_motion.ref_idx indexes that union (whoever flattens the picture renumbers
 * them; an I slice simply has no inter CUs) - and SAO / ALF on-off switches, which are resolved into the per-CTU records.                       */
#define VVR_SLICE_TOOL_MASK ( VVR_TOOL_DEP_QUANT | VVR_TOOL_LMCS | VVR_TOOL_LMCS_CSCALE | VVR_TOOL_SCALING_LIST | VVR_TOOL_WP )
typedef struct vvr_slice_header {
  uint32_t tool_flags;               /* this slice's value of the switches a slice header carries: VVR_TOOL_DEP_QUANT (sh_dep_quant_used_flag), VVR_TOOL_LMCS
                                        (sh_lmcs_used_flag), VVR_TOOL_LMCS_CSCALE (the picture's flag and sh_lmcs_used_flag), VVR_TOOL_SCALING_LIST
                                        (sh_explicit_scaling_list_used_flag), VVR_TOOL_WP (a P / B slice with weights); all other bits are ignored: those
                                        tools follow hdr.tool_flags                                                                                       */
  int8_t   deblock_beta_offset_div2[3];   /* Y, Cb, Cr: of the slice the deblocked CTU belongs to (LoopFilter.cpp:421,1473,1637)                        */
  int8_t   deblock_tc_offset_div2[3];
  uint8_t  slice_type;               /* 0 B, 1 P, 2 I (informative: the CUs say how they are predicted)                                                */
  uint8_t  alf_set;                  /* which of vvr_picture.alf_params[] holds the filters of the APSs this slice refers to (luma list, chroma, CC-ALF)   */
  uint8_t  wp_set;                   /* which of vvr_picture.wp[] holds this slice's pred_weight_table()                                               */
  uint8_t  pad[3];
} vvr_slice_header;

/* Reference picture resampling (RPR; sps_ref_pic_resampling_enabled_flag, scaling windows of the PPSs): how the current picture sees each of its
 * reference pictures.  A reference picture is "scaled" when its size or its scaling window differs from the current picture's (Picture::isRefScaled,
 * Picture.h:265); a prediction from such a picture is interpolated at positions that advance by the scaling ratio per sample, with low-pass filter
 * sets above ratios of 1.25 and 1.75 (InterPrediction::xPredInterBlkRPR, InterPrediction.cpp:2081-2217), its motion vectors are not clipped, and the
 * CU takes no BDOF, DMVR or PROF (InterPrediction.cpp:1431-1435,1029).  Indexed like hdr.ref_slot (the union of the slices' lists).  The DPB slot of a
 * scaled reference picture holds a picture of `width` x `height` luma samples in its top left corner (vvr_config.max_width / max_height bound every
 * picture of a context; a picture is reconstructed at hdr.width x hdr.height).
 * SbTMVP: every 8x8 sub-block is predicted on its own from the sub-block's position.  (The reference joins sub-blocks of equal motion unless the
 * slice's first reference pictures are scaled, InterPrediction.cpp:477; sub-block motion refers to the first reference picture of each list, so a
 * sub-block that reads a scaled picture is never part of a joined block.)
 * Not combined with reference wrap-around or with sub-pictures treated as pictures (the reference keeps no wrap copy of a scaled picture,
 * Picture.h:278, and a coded video sequence with such sub-pictures does not change its picture size).                                            */
typedef struct vvr_rpr_ref {
  int32_t  ratio[2];               /* Slice::getScalingRatio (CU::getRprScaling, UnitTools.cpp:92): x, y; 1 << 14 = same scale; 1 << 11 .. 1 << 15        */
  int32_t  win_left, win_top;      /* scaling window of the reference picture's PPS: left / top offset in luma samples (offset * SPS::getWinUnitX / Y)    */
  uint16_t width, height;          /* luma size of the reference picture                                                                                  */
  uint8_t  scaled;                 /* Picture::isRefScaled( current PPS )                                                                                 */
  uint8_t  hor_collocated_chroma;  /* sps_chroma_horizontal_collocated_flag / ..vertical.. of the reference picture's SPS (InterPrediction.cpp:2126)      */
  uint8_t  ver_collocated_chroma;
  uint8_t  pad;
} vvr_rpr_ref;
typedef struct vvr_rpr_params {
  int32_t     win_left, win_top;   /* scaling window of the current picture's PPS, luma samples                                                           */
  vvr_rpr_ref ref[2][VVR_MAX_REFS];
} vvr_rpr_params;

typedef struct vvr_picture {
  vvr_pic_header        hdr;
  uint32_t              num_cu, num_tu;
  const vvr_cu*         cu;            /* decode order (CTU raster, z-scan inside the CTU)                      */
  const vvr_tu*         tu;
  const uint32_t*       ctu_first_cu;  /* [num_ctu + 1] first CU of every CTU                                    */
  const int16_t*        coef;          /* packed quantised levels                                               */
  uint64_t              num_coef;
  const vvr_motion*     motion;        /* [h4][w4], may be NULL for intra pictures                               */
  const vvr_lfp*        lfp[2];        /* [EDGE_VER, EDGE_HOR][h4][w4]; not read with VVR_TOOL_LFP_ON_DEVICE        */
  const vvr_sao_ctu*    sao;           /* [num_ctu] or NULL                                                      */
  const vvr_alf_ctu*    alf;           /* [num_ctu] or NULL                                                      */
  const vvr_alf_params* alf_params;    /* NULL when ALF is off; [num_alf_sets] tables when slices refer to different APSs */
  const vvr_lmcs_params* lmcs;         /* NULL when LMCS is off                                                  */
  const vvr_wp_params*  wp;            /* NULL unless VVR_TOOL_WP; [num_wp_sets] tables when slices carry different weights */
  const vvr_scaling_list* scaling;     /* NULL unless VVR_TOOL_SCALING_LIST                                      */
  /* Slices and tiles.  The CTUs of the description are listed in picture raster order whatever order the bit stream coded them in.  Across a
   * slice or tile boundary nothing is available to intra prediction, CCLM or the LMCS chroma-scaling neighbourhood (CodingStructure::
   * getCURestricted, CodingStructure.cpp:464), and SAO / ALF stop there when the VVR_TOOL_NO_LF_ACROSS_* flag of the kind of boundary is set
   * (SampleAdaptiveOffset.cpp:741-830, AdaptiveLoopFilter.cpp:118-200).
   * Slices with headers of their own (ABI 4): `slices[ctu_slice[ctu]]` carries what a slice header can set differently from its neighbours -
   * see vvr_slice_header.  slices == NULL: every slice takes the values of `hdr` (and alf_params / wp are single tables). */
  const uint16_t*       ctu_slice;     /* [num_ctu] slice index of every CTU, NULL = one slice                   */
  const uint16_t*       ctu_tile;      /* [num_ctu] tile index of every CTU, NULL = one tile                     */
  /* Sub-pictures: rectangles of whole CTUs that tile the picture (NULL / 0 or 1: the picture is its only sub-picture).  Not combined with
   * reference wrap-around (the reference does not support the pair either, Picture.h:114).                                                   */
  const vvr_subpic*     subpics;
  uint32_t              num_subpics;
  const vvr_slice_header* slices;      /* [num_slices] or NULL                                                   */
  const vvr_rpr_params* rpr;           /* NULL: no reference picture of this picture is scaled (ABI 5)           */
  uint32_t              num_slices;    /* (ctu_slice values are < num_slices when slices != NULL)                */
  uint32_t              num_alf_sets;  /* entries of alf_params[] (0 or 1: one table), selected by vvr_slice_header.alf_set */
  uint32_t              num_wp_sets;   /* entries of wp[] (0 or 1: one table), selected by vvr_slice_header.wp_set          */
  int                   resident;      /* 0: all array pointers are host memory (copied H2D by vvr_submit);      */
                                       /* 1: all array pointers are DEVICE memory already resident in HBM        */
} vvr_picture;

/* ------------------------------------------------------------------------------------------------------------------
 * context  (replaces DecLibRecon instances + the DPB picture buffers they write)
 * ---------------------------------------------------------------------------------------------------------------- */
enum { VVR_STOP_NONE = 0, VVR_STOP_RECO = 1, VVR_STOP_DEBLOCK = 2, VVR_STOP_SAO = 3 };

typedef struct vvr_config {
  uint32_t abi_version;
  int32_t  device;               /* HIP device ordinal                                                          */
  uint16_t max_width, max_height;
  uint8_t  chroma_format, bit_depth, log2_ctu;
  uint8_t  num_slots;            /* DPB slots (pictures resident in HBM)                                        */
  uint8_t  num_streams;          /* pictures reconstructing concurrently (reference: 2, DecLib.h:70)            */
  uint8_t  host_threads;         /* worker threads that build the device work lists of submitted pictures (the reference spreads the set-up of
                                    decompressPicture over its thread pool, DecLibRecon.cpp:429-682).  0: the submitting thread does it inside
                                    vvr_submit; N > 0: vvr_submit only queues the picture, N pictures are prepared concurrently and enqueued
                                    on the device in submission order                                                                        */
  uint8_t  stop_after;           /* conformance aid (the reference has per-stage CRC traces for the same purpose, LoopFilter.cpp:399-406): 0 =
                                    full reconstruction; VVR_STOP_RECO / _DEBLOCK / _SAO: the pictures of this context stop after that stage, so
                                    that they can be compared with the reference's picture at the same point                                  */
  uint8_t  ring_entries;         /* entries of the upload ring (pinned staging + HBM image of one picture each); 0: 2 * num_streams +
                                    2 * host_threads + 4, enough for the pictures in the workers' hands plus those in flight on the device   */
  uint8_t  read_buffers;         /* pinned staging buffers of vvr_read_picture (one picture each) allocated with the context; 0: the first calls that
                                    need one allocate it (pinning 30 MB takes milliseconds: a decoder that reads every picture back asks for them here) */
  uint8_t  pad[7];
  void*    ext_planes;           /* optional: caller-owned device memory for the DPB, num_slots * vvr_slot_bytes */
                                 /* (mirrors vvdec_decoder_open_with_allocator, vvdec.h.in:576)                 */
} vvr_config;

typedef struct vvr_context vvr_context;

/* DecLibRecon::create (DecLibRecon.cpp:132): HIP streams/events, constant tables, DPB planes. */
VVR_API int          vvr_create(const vvr_config* cfg, vvr_context** out);
/* DecLibRecon::destroy */
VVR_API void         vvr_destroy(vvr_context* ctx);
/* DecLibRecon::decompressPicture (DecLibRecon.cpp:429): asynchronous; returns a job id >= 0 or an error code.  Called from ONE submitting
 * thread.  Header, tables and the set of arrays are validated before the call returns (with host_threads == 0 the CU / TU records as well);
 * the arrays the description points to must stay valid and unchanged until vvr_inputs_done(job) or vvr_wait(job) has returned (with
 * host_threads == 0 they are consumed before vvr_submit returns).  Errors that only show later (with worker threads: bad CU / TU records;
 * work lists; device) are parked on the job, the way the reference parks exceptions on reconDone, and come back from vvr_wait.  Pictures
 * take effect in submission order (one that shares no DPB slot with a picture still being prepared may be enqueued on the device ahead of
 * it); every job should eventually be waited for (vvr_wait / vvr_sync). */
VVR_API int          vvr_submit(vvr_context* ctx, const vvr_picture* pic);
/* blocks until the host arrays of job `job` are no longer needed (its device work lists are built and staged in pinned memory) */
VVR_API int          vvr_inputs_done(vvr_context* ctx, int job);
/* Host memory the device reads directly (pinned), owned by the context (freed with it at the latest).  A parser that writes its records into
 * such memory (the way vvdec_decoder_open_with_allocator, vvdec.h.in:576, lets the application own the picture buffers) saves the back-end the
 * staging copy: the cu / tu / coef / lfp arrays of a submitted picture that lie in it are copied to HBM from where they are, and must then stay
 * unchanged until vvr_inputs_done(job) (which waits for that copy) or vvr_wait(job). */
VVR_API void*        vvr_host_alloc(vvr_context* ctx, size_t bytes);
VVR_API void         vvr_host_free(vvr_context* ctx, void* p);
/* DecLibRecon::waitForPrevDecompressedPic (DecLibRecon.cpp:684): blocks until job `job` is reconstructed; returns its status. */
VVR_API int          vvr_wait(vvr_context* ctx, int job);
/* the same question without waiting (the ready check of a completion task on the decoder's thread pool, ThreadPool.cpp addBarrierTask: no pool
 * thread sleeps in vvr_wait): VVR_OK - job `job` is reconstructed (vvr_wait would return at once, with this status); VVR_NOT_READY - not yet;
 * negative - it failed.  The job stays to be waited for. */
VVR_API int          vvr_test(vvr_context* ctx, int job);
/* wait for everything in flight */
VVR_API int          vvr_sync(vvr_context* ctx);
/* geometry of a DPB slot: byte size, and per-plane offset / stride (bytes) / rows */
VVR_API size_t       vvr_slot_bytes(const vvr_config* cfg);
VVR_API int          vvr_plane_layout(const vvr_context* ctx, int comp, size_t* offset, size_t* stride_bytes, int* width, int* height);
/* device address of plane `comp` of `slot` (for zero-copy consumers, RCCL broadcast of reference pictures) */
VVR_API void*        vvr_plane_ptr(vvr_context* ctx, int slot, int comp);
/* vvdecFrame-style export (vvdecimpl.cpp:957 xAddPicture): copies plane `comp` of `slot` into a host buffer of 16-bit samples */
VVR_API int          vvr_read_plane(vvr_context* ctx, int slot, int comp, uint16_t* dst, size_t dst_stride_samples);
/* output of one plane the way the reference hands frames to the application (VVDecImpl::copyComp, vvdecimpl.cpp:818-880, called with the
 * conformance window applied): the window (x, y, w, h in samples of the component) is copied to dst with dst_stride_bytes between rows;
 * bytes_per_sample 2 = 16-bit samples, 1 = the low byte of every sample (8-bit streams; "only narrowing conversions", :853).  Crop and
 * narrowing run on the device: exactly w * h * bytes_per_sample bytes cross PCIe.  Waits for all work on the slot. */
VVR_API int          vvr_read_output(vvr_context* ctx, int slot, int comp, int x, int y, int w, int h, int bytes_per_sample, void* dst, size_t dst_stride_bytes);
/* the same window rescaled to out_w x out_h samples of the component, exactly as vvdec::rescalePlane does it (vvdecimpl.cpp:1620 ->
 * sampleRateConvCore, Buffer.cpp:235-318: the regular 8-tap / 4-tap DCTIF, scale factors from the window's and the output's sizes, source taps
 * clamped to the window), then stored like vvr_read_output.  collocated: bit 0 horizontal, bit 1 vertical chroma sample position
 * (horCollocatedChromaFlag / verCollocatedChromaFlag; 4:2:0 default of vvdecapp: 1); ignored for luma.  Output sides 1..8192, each between 1/8
 * and 8 times the window's; else VVR_ERR_PARAMETER.  The rescaling runs on the device: exactly out_w * out_h * bytes_per_sample bytes cross PCIe.
 * Waits for all work on the slot. */
VVR_API int          vvr_read_output_scaled(vvr_context* ctx, int slot, int comp, int x, int y, int w, int h, int out_w, int out_h,
                                            int collocated, int bytes_per_sample, void* dst, size_t dst_stride_bytes);

/* Film grain synthesis at the output (the VFGS "hardware model" of the reference's FilmGrain, FilmGrainImpl.cpp:126-324, as
 * VVDecImpl::xAddGrain applies it, vvdecimpl.cpp:897-956).  The bank is the model's state after FilmGrain::updateFGC, i.e. what the
 * "firmware" derives from an FGC SEI; parsing the SEI, cancel, persistence and the reset at a CLVS start stay with the caller. */
typedef struct vvr_film_grain_bank {
  uint32_t struct_size;                /* sizeof( vvr_film_grain_bank )                                                  */
  uint8_t  comp_present[3];            /* comp_model_present_flag[c]: absent components are copied unchanged             */
  uint8_t  shift;                      /* log2_scale_factor - ( model_id ? 1 : 0 ), 2..7                                 */
  uint8_t  scale_lut[3][256];          /* FilmGrainImpl::sLUT                                                            */
  uint8_t  pattern_lut[3][256];        /* FilmGrainImpl::pLUT (pattern index << 4, < 0x80)                               */
  int8_t   pattern[2][8][64][64];      /* [luma, chroma][index][row][col]; 4:2:0 chroma uses rows, cols < 32             */
} vvr_film_grain_bank;
/* the context's bank (copied; NULL: none).  A bank with a struct_size other than sizeof( vvr_film_grain_bank ), a shift outside 2..7 or a
 * pattern_lut entry >= 0x80 is refused (VVR_ERR_PARAMETER) and the bank set before stays.  Does not touch the seed chain. */
VVR_API int          vvr_set_film_grain(vvr_context* ctx, const vvr_film_grain_bank* bank);
/* FilmGrain::set_seed: the state of the seed chain (a context starts at 0xdeadbeef) */
VVR_API int          vvr_set_film_grain_seed(vvr_context* ctx, uint32_t seed);
/* one frame, all components: the window (x, y, w, h in luma samples of the picture in the slot; even in 4:2:0) with the bank's grain added,
 * stored like vvr_read_output into dst[c] at dst_stride_bytes[c] (dst[1], dst[2] unused in 4:0:0).  Per 16x16 block of the window (8x8 in
 * 4:2:0 chroma) a random word from the seed chain, which advances exactly as FilmGrain::prepareBlockSeeds( w, h ) does, and only when the call
 * succeeds; the output of a present component is clip( I + round( scale * grain, shift + 6 - ( bit_depth - 8 ) ), 0, 255 << ( bit_depth - 8 ) )
 * (so 1020 is the 10-bit ceiling).  Refused (VVR_ERR_PARAMETER): no bank, bit depth other than 8 or 10, w <= 128 (the reference's limits),
 * a window outside the picture or odd in 4:2:0, 1-byte output of a context with more than 8 bits.
 * Where the reference reads past the frame (the deblocking of the last block edge when the luma width is 1 mod 16 or the 4:2:0 chroma width
 * 1 mod 8: it takes the pattern index from the buffer's padding), the sample beyond the frame takes the pattern index of the frame's last
 * sample in the row.  The synthesis runs on the device in the same pass that crops and packs the window.  Waits for all work on the slot. */
VVR_API int          vvr_read_output_grain(vvr_context* ctx, int slot, int x, int y, int w, int h, int bytes_per_sample,
                                           void* const dst[3], const size_t dst_stride_bytes[3]);
/* Output queue: the three calls above as requests that are ordered behind the picture ON THE DEVICE and never drain the context (no
 * vvr_sync): a request runs on the context's output stream behind its picture's completion event, leaves through one of 8 ring entries
 * (device scratch + pinned staging, allocated on first use, grown on demand, freed by vvr_destroy) and is collected with its ticket.
 *   formats  VVR_OUT_PLANAR16 / VVR_OUT_PLANAR8: the bytes vvr_read_output / _scaled / _grain give for bytes_per_sample 2 / 1, same refusals;
 *            VVR_OUT_PACKED10: vvdecapp's packed output (--pyuv, _writeComponentToFile, vvdecHelper.h:106-145): every row of every plane is
 *            w / 4 * 5 bytes, samples s0..s3 the little-endian 40-bit word s0 | s1 << 10 | s2 << 20 | s3 << 30; a context of 8 bits stores
 *            s << 2 (:201-248).  Refused at bit depth 9 and when the output width of a plane is not a multiple of 4.
 *            VVR_OUT_NV12 / VVR_OUT_P010: the semi-planar forms display, encode and ML pipelines exchange.  Two planes leave the request: dst[0]
 *            takes the luma rows, dst[1] the interleaved chroma rows Cb0, Cr0, Cb1, Cr1, ... of 2 * ( out_w >> 1 ) samples, out_h >> 1 of them
 *            (dst_stride_bytes[1] covers that row; dst[2] and dst_stride_bytes[2] are ignored and may be NULL / 0).  NV12: one byte per sample,
 *            the sample itself in an 8-bit context; at 9 / 10 bits refused unless a narrowing is set (vvr_set_output_narrowing below).  P010: little-endian 16-bit words, sample << ( 16 - bit_depth ),
 *            bit depths 8, 9 and 10.  Both are refused in a 4:0:0 context: there is no chroma to interleave.
 *            VVR_OUT_RGB8 / VVR_OUT_RGB16 / VVR_OUT_RGBF16: planar R'G'B' for a model on the same GPU.  Three planes of out_w x out_h samples
 *            (or w x h) leave the request, dst[0], dst[1], dst[2] = R, G, B, rows of out_w * 1 (RGB8) or out_w * 2 bytes.  The frame that is
 *            converted is the one the other formats would store: the window, grained, rescaled.  The arithmetic is defined here to the bit:
 *              chroma to the luma grid: the 4-tap chroma DCTIF of vvr_read_output_scaled (1/32-sample table), its two passes and rounding.  Per
 *              direction, output position i reads the chroma plane at refPos = 16 * i - ( collocated ? 0 : 8 ) in 1/32 chroma samples (`collocated`
 *              of the request: bit 0 horizontal, bit 1 vertical), integer = refPos >> 5, frac = refPos & 31 (0 and 16, or 24 and 8), taps at
 *              integer - 1 .. integer + 2, each clamped to the chroma plane OF THE FRAME BEING CONVERTED; the horizontal sums are not normalised,
 *              the vertical pass runs over them, then ( sum + 2048 ) >> 12, clipped to [0, 2^bd - 1].
 *              matrix: od = 8 (RGB8) or bd; m = 2^od - 1, s = 2^( bd - 8 ); ( Kr, Kb ) from vvr_set_output_colour; Kg = 1 - Kr - Kb; limited
 *              range: ys = m / ( 219 s ), cs = m / ( 224 s ), yoff = 16 s; full range: ys = cs = m / ( 2^bd - 1 ), yoff = 0; coff = 2^( bd - 1 ).
 *              Five Q14 coefficients, computed once in double with q( v ) = floor( v * 16384 + 0.5 ): cy = q( ys ), rv = q( 2 ( 1 - Kr ) cs ),
 *              gu = -q( 2 Kb ( 1 - Kb ) / Kg * cs ), gv = -q( 2 Kr ( 1 - Kr ) / Kg * cs ), bu = q( 2 ( 1 - Kb ) cs ).  With y = Y - yoff,
 *              u = Cb' - coff, v = Cr' - coff in int32 and arithmetic shifts: R = clip( ( cy y + rv v + 8192 ) >> 14, 0, m ),
 *              G = clip( ( cy y + gu u + gv v + 8192 ) >> 14, 0, m ), B = clip( ( cy y + bu u + 8192 ) >> 14, 0, m ): within 0.5625 of the
 *              real-valued H.273 equations; 10 -> 8 bits is a rounding through the coefficients, not a truncation.
 *              RGB8: uint8.  RGB16: little-endian uint16, od = bd.  RGBF16: IEEE half, the RGB16 value v as half( float32( v ) * inv ) with
 *              inv = float32( 1 ) / float32( 2^bd - 1 ): one correctly rounded float32 multiply, one conversion rounding to nearest even.
 *            Refused: no colour description set, a 4:0:0 context (no chroma), a bit depth outside 8..10, an odd out_w or out_h, a missing plane
 *            among the three or a stride below the row.  Primaries and transfer conversion: vvr_set_output_transform below.
 *            VVR_OUT_RGBF32: the three planes as IEEE float32, rows of out_w * 4 bytes, for a model that takes ( 3, H, W ) float32 with a mean and a
 *            standard deviation per channel applied (vvr_set_output_normalisation below, where the value is defined to the bit).
 *            VVR_OUT_RGBA8 / _BGRA8 / _RGB24 / _BGR24 / _RGB10A2 / _RGBA16F: the same pixels interleaved, for a display surface, a compositor, an
 *            encoder's RGB input, an HDR swap chain, OpenCV- or PIL-style code.  One plane leaves the request, dst[0]; dst[1], dst[2] and their
 *            strides are ignored and may be NULL / 0.  A pixel in memory order, a row of out_w pixels:
 *              RGBA8   4 bytes  R, G, B, 255        BGRA8   4 bytes  B, G, R, 255        - the bytes VVR_OUT_RGB8 stores
 *              RGB24   3 bytes  R, G, B             BGR24   3 bytes  B, G, R             - the bytes VVR_OUT_RGB8 stores
 *              RGBA16F 8 bytes  four little-endian halves R, G, B, 0x3C00 (1.0)          - the halves VVR_OUT_RGBF16 stores
 *              RGB10A2 4 bytes  the little-endian dword R | G << 10 | B << 20 | 3 << 30.  Without a transform the matrix runs at od = 10
 *                      (m = 1023) for every bit depth 8, 9 and 10: the widening is a rounding through the coefficients, as the narrowing of RGB8 is.
 *                      Under a transform: ( Ek * 1023 + 32767 ) / 65535 in integer division, the correctly rounded 16 -> 10 bit reduction (65535
 *                      is odd: no ties).
 *            "the bytes X stores": the definition of X above and below, with or without a transform - RGB8's od = 8 without one and od = bd,
 *            ( Ek + 128 ) / 257 with one included.  The refusals are those of the three planar formats, a missing plane or a stride below the
 *            row among the planes the format uses.
 *            VVR_OUT_YUV444P8 / _YUV444P16 / _YUV422P8 / _YUV422P16 / _UYVY / _YUY2 / _Y210 / _V210 / _Y410: Y'CbCr with the chroma brought to
 *            4:4:4 or 4:2:2 on the device, for playout and capture hardware (packed 4:2:2), an encoder of a 4:2:2 / 4:4:4 transcode, a model or
 *            a filter that works in Y'CbCr on one grid.  The frame that is converted is the one every other format would store: the window,
 *            grained, rescaled, in that order.  No colour description is needed; transform, 3-D LUT and normalisation are ignored.  Y is the
 *            frame's luma unchanged.  With W = out_w (or w), H = out_h (or h):
 *              YUV444P8   dst[0..2] = Y, Cb', Cr', each W x H   rows of W bytes        the sample; above 8 bits: vvr_set_output_narrowing
 *              YUV444P16  the same                              rows of W * 2 bytes    the sample as a little-endian 16-bit word
 *              YUV422P8   Y W x H; Cb', Cr' ( W >> 1 ) x H      rows of W, W >> 1      as YUV444P8
 *              YUV422P16  the same                              W * 2, ( W >> 1 ) * 2  as YUV444P16
 *              UYVY       dst[0] alone, rows of W * 2 bytes     bytes Cb, Y0, Cr, Y1 per pixel pair; above 8 bits as YUV444P8
 *              YUY2       dst[0] alone, rows of W * 2 bytes     bytes Y0, Cb, Y1, Cr per pixel pair; above 8 bits as YUV444P8
 *              Y210       dst[0] alone, rows of W * 4 bytes     little-endian words Y0, Cb, Y1, Cr, each sample << ( 16 - bit_depth ) (P010's rule)
 *              V210       dst[0] alone, rows of ( ( W + 5 ) / 6 ) * 16 bytes: six pixels in four little-endian dwords.  With s' = sample <<
 *                         ( 10 - bit_depth ) (VVR_OUT_PACKED10's widening) and Cbk, Crk the chroma of pixel pair k of the group:
 *                           d0 = Cb0 | Y0 << 10 | Cr0 << 20      d1 = Y1 | Cb1 << 10 | Y2 << 20
 *                           d2 = Cr1 | Y3 << 10 | Cb2 << 20      d3 = Y4 | Cr2 << 10 | Y5 << 20
 *                         bits 30 and 31 are 0.  W is even: the last group of a row holds 2, 4 or 6 pixels; the fields of pixels that do not
 *                         exist are 0 and the whole 16-byte group is stored.  The conventional padding of a line to 128 bytes is the caller's
 *                         dst_stride_bytes[0]: the request only requires the stride to cover the row above.
 *              Y410       dst[0] alone, rows of W * 4 bytes     the little-endian dword Cb' | Y << 10 | Cr' << 20 | 3 << 30 per pixel, 4:4:4,
 *                         values sample << ( 10 - bit_depth )
 *            For the one-plane formats dst[1], dst[2] and their strides are ignored and may be NULL / 0.  The chroma is the arithmetic of the
 *            RGB formats, not a new one:
 *              4:4:4 (YUV444P8, YUV444P16, Y410): Cb' and Cr' are exactly the "chroma to the luma grid" planes above - the same positions
 *              16 * i - ( collocated ? 0 : 8 ) per direction, the same taps clamped to the chroma plane of the frame being converted, the
 *              horizontal sums not normalised, the vertical pass over them, then ( sum + 2048 ) >> 12 clipped to [0, 2^bd - 1].  The matrix
 *              of VVR_OUT_RGB16 applied to ( Y, Cb', Cr' ) gives the planes VVR_OUT_RGB16 stores.
 *              4:2:2 (YUV422P8 ... V210): the same two passes with the horizontal position 32 * i - phase 0 at every i, tap set ( 0, 64, 0, 0 ),
 *              so the horizontal sum is 64 times the sample - and the vertical pass as above with bit 1 of `collocated`.  That is
 *              clip( ( c0 s0 + c1 s1 + c2 s2 + c3 s3 + 32 ) >> 6, 0, 2^bd - 1 ) with the four taps of the row's phase over the chroma rows
 *              integer - 1 .. integer + 2 of the same column, clamped to the plane: what the kernel computes.  Bit 0 of `collocated` is
 *              ignored: the horizontal chroma grid is the stream's.  With a collocated vertical position every second row is the source row.
 *            Refused, each with its text, before a ring entry is taken: a 4:0:0 context (no chroma to upsample); an 8-bit format in a context
 *            of more than 8 bits with no narrowing set (vvr_set_output_narrowing below); a bit depth outside 8..10; an odd out_w or out_h; a missing
 *            plane or a stride below the row among the planes the format uses.
 *            Not offered: semi-planar 4:2:2 / 4:4:4 (P210, NV16), AYUV / VUYA, Y216 / Y416; 4:0:0 with neutral
 *            chroma; these formats from the synchronous vvr_read_output* calls; decoding 4:2:2 / 4:4:4 streams.
 *            Not offered: interleaved float32; 4:0:0 as grey; RGB from the synchronous vvr_read_output* calls; constant-luminance BT.2020,
 *            ICtCp, YCgCo, the identity matrix; a 3-D LUT for the synchronous calls.  Dynamic metadata: the per-frame measurements exist
 *            (vvr_stats_submit, vvr_light_level below); parsing ST 2094 / CLL SEIs, smoothing over time and scene logic do not.
 *   grain with out_w / out_h: the window is grained at its own size exactly as vvr_read_output_grain does it, the grained frame is then
 *            rescaled exactly as vvr_read_output_scaled rescales a picture, taps clamped to the grained frame (the reference's order:
 *            xAddGrain in xAddPicture, then the application's upscaleFrame).
 *   seed chain: shared with vvr_read_output_grain; it advances in vvr_output_submit, in submission order, for accepted requests only.
 *   slot     the request reads `slot` until its kernels have run (tens of microseconds; NOT until the copy to the host has finished): pictures
 *            submitted (vvr_submit) after vvr_output_submit has returned a ticket that overwrite the slot are ordered behind that on the device.
 *            The other way round is the caller's duty: a request is submitted BEFORE the next picture into its slot is (one that comes after that
 *            picture has been handed to the device is refused; one that races with it gets whichever picture the slot holds).
 *   dst      when every dst[c] lies in memory of vvr_host_alloc the device copies straight there at the caller's stride and vvr_output_wait
 *            copies nothing; else the rows leave pinned staging inside vvr_output_wait, on the waiting thread.  Either way exactly the
 *            output's bytes cross PCIe.  dst must stay valid until vvr_output_wait has returned.
 *   dst on the device   when every plane the request uses (dst[0], dst[1] of the semi-planar formats, else all planes) lies wholly inside a
 *            range of vvr_device_alloc / vvr_device_register, the request is a device request: nothing crosses PCIe, every format is accepted,
 *            vvr_output_wait copies nothing.  A plane whose rows are back to back (dst_stride_bytes[k] equal to the row's bytes) at a base
 *            aligned to 32 bytes is stored by the last kernel itself, exactly its bytes; any other plane is laid out at the caller's stride by
 *            one device-to-device copy.  No byte outside the rows changes.  A plane partly inside a range, and device planes mixed with host
 *            planes, are refused.  The caller's duty: the destination is memory of the context's device, it is idle when the request is
 *            submitted, and nothing touches it before the request has completed (vvr_output_wait / vvr_output_test on the host,
 *            vvr_output_stream_wait on the device).
 * vvr_output_submit: a ticket (>= 2: never VVR_NOT_READY); VVR_ERR_PARAMETER (with a text) for a request that is refused; VVR_ERR_BUSY when 8 requests are in flight;
 *   VVR_NOT_READY (blocking == 0) when `job` has not been handed to the device yet.  A request for a job that failed is accepted and fails with
 *   the job's status from vvr_output_test / vvr_output_wait.  vvr_output_test: VVR_OK (vvr_output_wait returns at once) / VVR_NOT_READY / the
 *   failure; the ticket stays.  vvr_output_wait blocks for THIS request only and retires the ticket.  An unknown or retired ticket:
 *   VVR_ERR_PARAMETER.  vvr_sync also waits for the requests in flight but retires no ticket. */
enum { VVR_OUT_PLANAR16 = 0, VVR_OUT_PLANAR8 = 1, VVR_OUT_PACKED10 = 2, VVR_OUT_NV12 = 16, VVR_OUT_P010 = 17, VVR_OUT_RGB8 = 32, VVR_OUT_RGB16 = 33, VVR_OUT_RGBF16 = 34,
       VVR_OUT_RGBF32 = 36, VVR_OUT_RGBA8 = 48, VVR_OUT_BGRA8 = 49, VVR_OUT_RGB24 = 50, VVR_OUT_BGR24 = 51, VVR_OUT_RGB10A2 = 52, VVR_OUT_RGBA16F = 53,
       VVR_OUT_YUV444P8 = 64, VVR_OUT_YUV444P16 = 65, VVR_OUT_YUV422P8 = 66, VVR_OUT_YUV422P16 = 67, VVR_OUT_UYVY = 68, VVR_OUT_YUY2 = 69, VVR_OUT_Y210 = 70,
       VVR_OUT_V210 = 71, VVR_OUT_Y410 = 72 };
typedef struct vvr_output_request {
  uint32_t struct_size;        /* sizeof( vvr_output_request ) */
  int32_t  slot;
  int32_t  job;                /* >= 0: the picture this job reconstructs into `slot`, ordered behind it ON THE DEVICE;
                                  -1: the slot as all work submitted so far leaves it (vvr_stream_wait_slot's rule) */
  int32_t  x, y, w, h;         /* window, luma samples (even in 4:2:0) */
  int32_t  out_w, out_h;       /* 0, 0: the window's size; else rescaled as vvr_read_output_scaled does it (chroma: >> 1), or resampled by the filter of vvr_set_output_resampling */
  uint8_t  collocated;         /* as vvr_read_output_scaled */
  uint8_t  format;             /* VVR_OUT_* */
  uint8_t  grain;              /* 1: the context's bank is added first, one frame of the seed chain (vvr_read_output_grain's rules) */
  uint8_t  blocking;           /* 0: VVR_NOT_READY instead of waiting on the host until `job` has been handed to the device */
  void*    dst[3];             /* dst[1], dst[2] unused in 4:0:0; dst[2] unused by VVR_OUT_NV12 / VVR_OUT_P010; R, G, B for the planar VVR_OUT_RGB*; Y, Cb, Cr for VVR_OUT_YUV4*P*; dst[0] alone for the interleaved and the packed Y'CbCr ones */
  size_t   dst_stride_bytes[3];
} vvr_output_request;
/* the colour description the RGB formats convert with - context state, like the film grain bank; a new context has none.  matrix_coefficients
 * is the H.273 code point: 1 (BT.709), 5 or 6 (BT.601), 9 (BT.2020 non-constant luminance); full_range is video_full_range_flag, 0 or 1.
 * Anything else - 0 (identity / GBR), 2 (unspecified: the caller decides), 14, ... - is VVR_ERR_PARAMETER with a text, and the value set before
 * stays.  A request takes the value that is set when vvr_output_submit accepts it: the coefficients travel as kernel arguments, a later call
 * never changes a request in flight. */
VVR_API int          vvr_set_output_colour(vvr_context* ctx, int matrix_coefficients, int full_range);
/* 8-bit Y'CbCr frames from 9- and 10-bit pictures - context state, like the colour description.  mode: VVR_NARROW_REFUSE (a new context: the
 * byte-per-sample formats are refused above 8 bits, as ever), _TRUNCATE, _ROUND or _DITHER; phase: 0 .. 3.  A mode outside 0 .. 3 or a phase
 * outside 0 .. 3 is VVR_ERR_PARAMETER with a text, and the value set before stays.  A request takes the value that is set when
 * vvr_output_submit accepts it: the values travel as kernel arguments, a later call never changes a request in flight.
 *   The mode is looked at only for the six byte-per-sample Y'CbCr formats - VVR_OUT_PLANAR8, _NV12, _YUV444P8, _YUV422P8, _UYVY, _YUY2 - and only
 *   in a context of 9 or 10 bits.  In an 8-bit context, and for every other format, a request stores exactly the bytes it stores with mode 0.
 *   Defined to the bit.  s = bit_depth - 8 (1 or 2); v: the 16-bit word the 16-bit sibling format would store for the sample - VVR_OUT_PLANAR16
 *   for PLANAR8 and NV12, _YUV444P16 for YUV444P8, _YUV422P16 for YUV422P8, UYVY and YUY2 - that is the window, grained, rescaled, with the
 *   chroma upsampled, in that order; the reduction is the very last step before the store.  In 32-bit arithmetic:
 *     byte = min( 255, ( v + a ) >> s )
 *     TRUNCATE  a = 0                     (at 10 bits what vvdecapp writes for an 8-bit file of a 10-bit stream, vvdecHelper.h:90)
 *     ROUND     a = 1 << ( s - 1 )
 *     DITHER    a = M[ ( j + ( phase >> 1 & 1 ) ) & 1 ][ ( i + ( phase & 1 ) ) & 1 ] >> ( 2 - s ),   M = { { 0, 2 }, { 3, 1 } }
 *   ( i, j ): the sample's column and row IN ITS OWN OUTPUT PLANE - the stored frame's, not the picture's.  Luma: ( x, y ).  A chroma plane of
 *   PLANAR8 / NV12: its own 4:2:0 coordinates; the Cb and the Cr of NV12's pair k in row j both use ( k, j ).  YUV444P8 chroma: ( x, y ).
 *   YUV422P8 / UYVY / YUY2 chroma of pixel pair k: ( k, y ).  The min matters in every mode but TRUNCATE on in-range samples:
 *   ( 1023 + 3 ) >> 2 = 256.  v is read as it lies (vvr_write_plane can put anything into a slot); clamping v to 2^bit_depth - 1 first gives
 *   the same byte for every input, and the packed 16-bit arithmetic of the device relies on it.  `phase` lets a caller move the pattern per
 *   frame; nothing in the library advances it.
 *   Everything vvr_output_submit refuses stays refused under a mode: the 4:0:0 refusals of NV12 and the 4:2:2 / 4:4:4 formats, grain at depths
 *   other than 8 and 10, odd sizes, ...  PLANAR8 of a 4:0:0 context at 9 / 10 bits is accepted, luma alone.
 *   Not offered: the synchronous vvr_read_output* calls with bytes_per_sample == 1 keep their refusal above 8 bits; error diffusion and
 *   blue-noise masks; dither for the RGB formats; P210 / NV16. */
enum { VVR_NARROW_REFUSE = 0, VVR_NARROW_TRUNCATE = 1, VVR_NARROW_ROUND = 2, VVR_NARROW_DITHER = 3 };
VVR_API int          vvr_set_output_narrowing(vvr_context* ctx, int mode, int phase);
/* Antialiased resampling for out_w / out_h - context state, like the narrowing.  filter: VVR_RESAMPLE_REFERENCE (a new context: the rescale
 * step is vvdec::rescalePlane's DCTIF as ever - same bytes, same refusals, same texts), _AREA, _TRIANGLE (what torch's interpolate( mode =
 * "bilinear", antialias = True ) and PIL's BILINEAR compute) or _CUBIC (Keys, a = -1/2: torch's "bicubic" with antialias, PIL's BICUBIC).  A
 * value outside 0 .. 3 is VVR_ERR_PARAMETER with a text, and the value set before stays.  A request takes the value that is set when
 * vvr_output_submit accepts it; a later call never changes a request in flight.
 *   With a filter set the rescale step of vvr_output_submit's chain (window -> grain -> rescale -> format) is k_output_resample, for every
 *   format and every kind of destination; everything behind it reads the resampled 4:2:0 frame exactly as it reads the rescaled one.  The
 *   accepted range becomes, per plane and axis, n <= 64 m and m <= 8 n with m >= 1 (n source, m output samples; chroma sizes are >> 1 of the
 *   window's and of the output's; output sides stay 1 .. 8192).  A request outside it is refused with a text naming the limit before a ring
 *   entry is taken or the seed chain advances.
 *   Defined to the bit, in integers.  Each plane is resampled on its own, horizontally then vertically.  Per axis: n is the number of source
 *   samples of the frame being converted (the window, after grain if `grain` is set), m the number of output samples; phi = 2 for luma and
 *   for chroma whose `collocated` bit of that axis is 0, phi = 1 for chroma whose bit is 1 (the output keeps the siting of the source).  With
 *   g = gcd( n, m ), n' = n / g, m' = m / g:
 *     P_k = ( 4 k + phi ) m'      Q_i = ( 4 i + phi ) n'      S = 4 max( n', m' )      N = | P_k - Q_i |
 *   (the weights do not change under the division by g; it keeps every integer below inside 64 bits: 4 S^3 * 32768 < 2^63 for S <= 32768).
 *   Numerator of source sample k for output sample i:
 *     TRIANGLE  S - N where N < S
 *     CUBIC     3 N^3 - 5 N^2 S + 2 S^3 where N < S;  - N^3 + 5 N^2 S - 8 N S^2 + 4 S^3 where S <= N < 2 S (may be 0 or negative)
 *     AREA      the length of the overlap of the output footprint [ Q_i - 2 n', Q_i + 2 n' ) with the box of sample k,
 *               [ P_k - 2 m', P_k + 2 m' ); the box of sample 0 reaches to minus infinity, the box of sample n - 1 to plus infinity, so the
 *               numerators always sum to 4 n'
 *   Taps: the samples 0 <= k < n with N < S (TRIANGLE), N < 2 S (CUBIC), a positive overlap (AREA).  They form one run first .. first +
 *   count - 1 with count <= VVR_RESAMPLE_MAX_TAPS.  Samples beyond the plane are dropped, not clamped - the renormalisation torch and PIL do,
 *   which is why the edges agree with them.
 *   Weights: T is the sum of the kept numerators (positive); w_k = floor( ( 2 num_k 16384 + T ) / ( 2 T ) ), the floor towards minus
 *   infinity; then 16384 - sum( w_k ) is added to the largest w_k, the lowest k among equals.  Every tap list sums to exactly 16384 and a flat
 *   plane stays flat.
 *   Horizontal pass, for every source row r:   H[r][i] = ( sum_k wx[i][k] s[r][k] + 512 ) >> 10      (arithmetic shift; four fractional bits, not clipped)
 *   Vertical pass:                        out[j][i] = clip( ( sum_r wy[j][r] H[r][i] + 131072 ) >> 18, 0, 2^bd - 1 )
 *   All sums are in int32: integer sums, so any order and any tiling give the same bits; the rounding of H is per sample.
 *   vvr_resample_taps: a host helper like vvr_xpsnr_blocks - the taps of output sample i of one axis (phase: the phi above, 1 or 2) into
 *   *first and weights[0 .. count - 1]; returns count, or VVR_ERR_PARAMETER for filter 0 or an unknown filter, sizes outside the accepted range
 *   (1 <= n, m <= 8192, n <= 64 m, m <= 8 n), a phase other than 1 or 2, i outside 0 .. m - 1, or a NULL pointer.
 *   Not offered: Lanczos, Mitchell, Gaussian and other kernels; ratios beyond 1/64; the filters for vvr_read_output_scaled and the other
 *   synchronous calls, for vvr_set_compare_scaling, for statistics and hashes - those keep the reference's DCTIF (or read the picture as it
 *   lies) whatever is set here. */
enum { VVR_RESAMPLE_REFERENCE = 0, VVR_RESAMPLE_AREA = 1, VVR_RESAMPLE_TRIANGLE = 2, VVR_RESAMPLE_CUBIC = 3 };
#define VVR_RESAMPLE_MAX_TAPS 256
VVR_API int          vvr_set_output_resampling(vvr_context* ctx, int filter);
VVR_API int          vvr_resample_taps(int filter, int n, int m, int phase, int i, int32_t* first, int16_t weights[VVR_RESAMPLE_MAX_TAPS]);   /* returns count, or VVR_ERR_PARAMETER */
/* Normalisation of VVR_OUT_RGBF32: a mean and a standard deviation per channel (R, G, B), as a vision model takes them.  Context state like the
 * colour description (copied; NULL, NULL: none; a new context has none): a VVR_OUT_RGBF32 request takes the value that is set when
 * vvr_output_submit accepts it, it travels as kernel arguments, a later call never changes a request in flight.  Every other format -
 * VVR_OUT_RGBF16 and VVR_OUT_RGBA16F too - ignores it.  Defined to the bit:
 *   v        the value VVR_OUT_RGB16 stores for the channel, 0 .. M: M = 2^bd - 1 without a transform or a 3-D LUT, 65535 with either.
 *   scale[c] = (float)( 1.0 / ( (double) M * (double) std[c] ) ), bias[c] = (float)( -(double) mean[c] / (double) std[c] ): computed on the host in
 *            double, rounded once.  None set: scale[c] = (float)( 1.0 / M ), bias[c] = +0.
 *   t = float32( v ) * scale[c], one correctly rounded float32 multiply; out = t + bias[c], one correctly rounded float32 add; never an FMA.
 * Refused (VVR_ERR_PARAMETER with a text, the value set before stays in force): one of the two pointers NULL, an entry that is not finite, a
 * std[c] outside [ 2^-20, 2^20 ], a | mean[c] | above 2^20.  Within these bounds no product, sum or result is subnormal: the result does not
 * depend on a denormal mode. */
VVR_API int          vvr_set_output_normalisation(vvr_context* ctx, const float mean[3], const float std[3]);
/* Linear-light colour transform of the RGB formats: 1-D table -> 3x3 matrix -> 1-D table, the shaper / matrix / shaper of colour management and the
 * degamma / CTM / gamma of a display controller - what brings PQ- or HLG-coded BT.2020 R'G'B' to sRGB or BT.709 for a model, a display path or a
 * thumbnailer.  Context state like the colour description (copied; NULL: none; a new context has none).  It runs inside the RGB request's one
 * kernel, in registers, between the Y'CbCr matrix above and the store.  The integer pipeline is defined here to the bit; the floating-point
 * colour science lives only in how the tables are filled (vvr_output_transform_preset fills them for the standard cases, the caller keeps the
 * choice of any other tone curve).
 *   which requests   a request of any RGB format (planar or interleaved) takes the transform that is set when vvr_output_submit accepts it (the rule of the
 *            colour description): the tables are refreshed on the output stream ahead of the request's kernel, the matrix travels as kernel
 *            arguments, so a later vvr_set_output_transform never changes a request in flight.  Every other format ignores the transform, and so
 *            does every synchronous call.
 *   input    ( r, g, b ): the three values of the definition above computed at od = bd - also for VVR_OUT_RGB8, whose Y'CbCr matrix runs at
 *            od = bd under a transform - each 0 .. 2^bd - 1.
 *   stage 1  Lc = lin[c] for c in r, g, b.  lin[v] belongs to the R'G'B' value v (what a plain VVR_OUT_RGB16 request stores); the first 2^bd
 *            entries are read.
 *   stage 2  in int64 with an arithmetic shift: Tk = clip( ( m[k][0] * Lr + m[k][1] * Lg + m[k][2] * Lb + 8192 ) >> 14, 0, 65535 ), k = 0, 1, 2.
 *            m is Q14, every | m[k][j] | <= 65536 (4.0).  Three products of 65536 x 65535 do not fit 32 bits: the sum is 64 bits wide.
 *   stage 3  i = Tk >> 6, f = Tk & 63, Ek = ( enc[i] * ( 64 - f ) + enc[i + 1] * f + 32 ) >> 6, 0 .. 65535: enc[i] belongs to the stage-2 value
 *            64 * i (enc[1024] to 65536, which is never reached: it only closes the last interval), linear interpolation between entries.
 *   store    RGB8: ( Ek + 128 ) / 257, the correctly rounded 16 -> 8 bit reduction (65535 = 255 x 257).  RGB16: Ek itself - under a transform
 *            VVR_OUT_RGB16 is full-scale 16 bits, not bd bits.  RGBF16: half( float32( Ek ) * inv ) with inv = float32( 1 ) / float32( 65535 ):
 *            one correctly rounded float32 multiply, one conversion rounding to nearest even, as without a transform.
 * Refused (VVR_ERR_PARAMETER with a text, the value set before stays in force): a struct_size other than sizeof( vvr_output_transform ), a matrix
 * entry beyond +-65536.  A transform may be set in any context: it only ever meets RGB requests, and a 4:0:0 context refuses those. */
typedef struct vvr_output_transform {
  uint32_t struct_size;      /* sizeof( vvr_output_transform ) */
  uint32_t pad;
  uint16_t lin[1024];        /* stage 1: entry v for the R'G'B' value v at od = bd (what VVR_OUT_RGB16 stores); the first 2^bd entries are read */
  int32_t  m[3][3];          /* stage 2: Q14, every |m| <= 65536 (4.0) */
  uint16_t enc[1025];        /* stage 3: entry i belongs to the stage-2 value 64 * i */
  uint16_t pad2[3];
} vvr_output_transform;
VVR_API int          vvr_set_output_transform(vvr_context* ctx, const vvr_output_transform* t);
/* The tables for HDR video to BT.709 primaries (D65), filled in double precision; a pure host function, no context.  q16( v ) = floor( v * 65535 + 0.5 ).
 *   transfer_characteristics (H.273)  16: PQ, 18: HLG.  colour_primaries (H.273), the source gamut  9: BT.2020, 1: BT.709.
 *   target   VVR_XFORM_TO_SRGB, VVR_XFORM_TO_BT709 (the BT.709 OETF) or VVR_XFORM_TO_LINEAR; the target gamut is always BT.709's.
 *   bit_depth  8, 9 or 10: the context's; lin[v] is filled for v <= 2^bit_depth - 1 with E' = v / ( 2^bit_depth - 1 ), the rest is 0.
 *   PQ: lin[v] = q16( min( EOTF( EETF( E' ) ) / dst_peak_nits, 1 ) ).
 *            EOTF (SMPTE ST 2084, BT.2100-2 table 4): 10000 * ( max( E'^( 1 / m2 ) - c1, 0 ) / ( c2 - c3 * E'^( 1 / m2 ) ) )^( 1 / m1 ) cd/m2, m1 = 2610 / 16384,
 *            m2 = 2523 / 4096 * 128, c1 = 3424 / 4096, c2 = 2413 / 4096 * 32, c3 = 2392 / 4096 * 32; its inverse I( L ) = ( ( c1 + c2 Y ) / ( 1 + c3 Y ) )^m2, Y = ( L / 10000 )^m1.
 *            EETF (BT.2390-10 section 5.4.1, per channel, mastering black and target black 0): lo = I( 0 ), hi = I( src_peak_nits ),
 *            E1 = clip( ( E' - lo ) / ( hi - lo ), 0, 1 ), maxLum = ( I( dst_peak_nits ) - lo ) / ( hi - lo ), KS = 1.5 maxLum - 0.5; E2 = E1 when
 *            E1 < KS or KS >= 1, else the Hermite spline ( 2 T^3 - 3 T^2 + 1 ) KS + ( T^3 - 2 T^2 + T ) ( 1 - KS ) + ( -2 T^3 + 3 T^2 ) maxLum with
 *            T = ( E1 - KS ) / ( 1 - KS ); the black lift b ( 1 - E2 )^4 is 0; EETF = E2 ( hi - lo ) + lo.  Both peaks in ( 0, 10000 ].
 *   HLG: lin[v] = q16( inverse OETF( E' ) ) (BT.2100-2 table 5): E'^2 / 3 for E' <= 1/2, else ( exp( ( E' - c ) / a ) + b ) / 12, a = 0.17883277,
 *            b = 1 - 4 a, c = 0.5 - a ln( 4 a ): scene light 0 .. 1.  The two peaks are ignored: this is the scene-referred conversion of
 *            BT.2408 (section 5.1 of BT.2408-7: no OOTF, no system gamma), not a display-referred one.
 *   m[k][j] = floor( M[k][j] * 16384 + 0.5 ), M = inverse( N709 ) * Nsrc, N the normalised primary matrix RGB -> XYZ of a gamut (SMPTE RP 177: the
 *            columns x / y, 1, ( 1 - x - y ) / y of R, G, B scaled so that R = G = B = 1 gives the white point with Y = 1) from the chromaticities of
 *            BT.2020-2 table 3 (0.708, 0.292; 0.170, 0.797; 0.131, 0.046) and BT.709-6 item 1.3 (0.640, 0.330; 0.300, 0.600; 0.150, 0.060), D65 =
 *            (0.3127, 0.3290).  Source primaries 1: the identity.  BT.2020: 27205 -9628 -1194 / -2041 18561 -137 / -297 -1648 18329 (the matrix of BT.2407 section 2.2, the inverse of BT.2087's M2).
 *   enc[i] = q16( OETF( min( 64 i, 65535 ) / 65535 ) ).  sRGB (IEC 61966-2-1): 12.92 L for L <= 0.0031308, else 1.055 L^( 1 / 2.4 ) - 0.055.
 *            BT.709 (BT.709-6 item 1.2): 4.5 L for L < 0.018, else 1.099 L^0.45 - 0.099.  Linear: min( 64 i, 65535 ).
 * struct_size and the pads are set.  Any other code point, target, bit depth or peak: VVR_ERR_PARAMETER, *out untouched. */
enum { VVR_XFORM_TO_SRGB = 0, VVR_XFORM_TO_BT709 = 1, VVR_XFORM_TO_LINEAR = 2 };
VVR_API int          vvr_output_transform_preset(vvr_output_transform* out, int transfer_characteristics, int colour_primaries, int target,
                                                 double src_peak_nits, double dst_peak_nits, int bit_depth);
/* 3-D LUT of the RGB formats, tetrahedral interpolation: what a per-channel transform cannot express - a tone curve on luminance that keeps hue
 * and saturation (the BT.2390 EETF on Y, the HLG OOTF with its system gamma), or any grade a colour tool exports as a .cube file.  Context state
 * like the transform (copied inside the call; NULL with n = 0: none; a new context has none).  It runs inside the RGB request's one kernel, last
 * before the store, behind the transform if one is set.  Defined to the bit:
 *   nodes    n = 17, 33 or 65 per axis; n^3 x 3 values in .cube order, R fastest: node ( jr, jg, jb ) at 3 * ( ( jb * n + jg ) * n + jr ), as R, G, B.
 *   which requests   a request of any RGB format (planar or interleaved) takes the LUT that is set when vvr_output_submit accepts it: the nodes
 *            are refreshed on the output stream ahead of the request's kernel, the size travels as a kernel argument, so a later
 *            vvr_set_output_lut3d never changes a request in flight.  Every other format ignores the LUT, and so does every synchronous call.
 *            The refresh travels through the ring entry's pinned staging, as the transform's tables do: the first RGB request behind a changed
 *            LUT may grow its entry's staging by the nodes (8 n^3 bytes: 39 KB, 287 KB, 2.2 MB) inside vvr_output_submit, once per entry -
 *            what a request with a larger output than the entry has seen does too.  A caller that changes a 65-point LUT per frame pays that
 *            once for each of the 8 entries, and the upload of 2.2 MB each time.
 *   input    with a transform: the three Ek of stage 3, each 0 .. 65535.  Without one: the Y'CbCr matrix runs at od = bd - also for VVR_OUT_RGB8 and
 *            VVR_OUT_RGB10A2, as it does under a transform - and each value v is widened to ( v * 65535 + ( M >> 1 ) ) / M, M = 2^bd - 1, in
 *            integer division: the correctly rounded widening.
 *   cell     s = 16 - log2( n - 1 ) (12, 11, 10), S = 2^s; per channel i = v >> s (0 .. n - 2), f = v & ( S - 1 ).  Node j belongs to the value
 *            j * S (node n - 1 to 65536, which is never reached: it only closes the last cell - the convention of enc[1024]).
 *   interpolation    order the three fractions f1 >= f2 >= f3.  c0 = node ( ir, ig, ib ); c1 = c0 stepped by one along the axis of f1; c2 = c1
 *            stepped along the axis of f2; c3 = node ( ir + 1, ig + 1, ib + 1 ).  Per output channel k:
 *            Ok = ( c0[k] * ( S - f1 ) + c1[k] * ( f1 - f2 ) + c2[k] * ( f2 - f3 ) + c3[k] * f3 + ( S >> 1 ) ) >> s.  The weights sum to S: the sum
 *            stays below 2^28.  Equal fractions need no rule: the vertex that differs has weight 0.
 *   store    exactly the stores under a transform with Ek := Ok: RGB8 / RGBA8 / RGB24 (and the BGR orders) ( Ok + 128 ) / 257, RGB10A2
 *            ( Ok * 1023 + 32767 ) / 65535, RGB16 full-scale 16 bits, the halves and float32 with M = 65535.
 * Refused (VVR_ERR_PARAMETER with a text, the LUT set before stays in force): an n other than 17, 33, 65; nodes == NULL with n != 0.  A LUT may be
 * set in any context. */
enum { VVR_LUT3D_MAX = 65 };
VVR_API int          vvr_set_output_lut3d(vvr_context* ctx, int n, const uint16_t* nodes);
/* The nodes for HDR video to BT.709 primaries with the tone curve on luminance; a pure host function, no context, everything in double.  Meant
 * for use WITHOUT a transform: the LUT's input is the coded R'G'B'.  Code points, targets and the PQ peaks: those of vvr_output_transform_preset,
 * whose q16, EOTF, I, EETF, OETFs and gamut matrix M these are; n = 17, 33 or 65.  Per node E'c = min( jc * S, 65535 ) / 65535, c in R, G, B.
 *   PQ:   Lc = EOTF( E'c ); Y = sum of w_c * Lc, w the middle row of the source gamut's normalised primary matrix; if Y > 0:
 *         Lc *= EOTF( EETF( I( Y ) ) ) / Y - the BT.2390 curve on luminance, hue and saturation kept; Lc /= dst_peak_nits.
 *   HLG:  Ec = inverse OETF( E'c ); Ys = sum of w_c * Ec; Fc = Ys^( gamma - 1 ) * Ec (0 at Ys = 0), gamma = 1.2 + 0.42 log10( Lw / 1000 ) for
 *         400 <= Lw <= 2000, else 1.2 * 1.111^log2( Lw / 1000 ) (BT.2100-2 note 5f, BT.2390-10 section 6.2), Lw = dst_peak_nits;
 *         src_peak_nits is ignored.  One difference from vvr_output_transform_preset, which ignores both peaks for HLG: here dst_peak_nits
 *         is the display's peak and must lie in ( 0, 10000 ] - the system gamma has no value at Lw <= 0.
 *   both: T = M * L (or F), clipped to [ 0, 1 ]; node[k] = q16( OETF( Tk ) ).
 * Anything else: VVR_ERR_PARAMETER, nodes untouched. */
VVR_API int          vvr_output_lut3d_preset(uint16_t* nodes, int n, int transfer_characteristics, int colour_primaries, int target,
                                             double src_peak_nits, double dst_peak_nits);
VVR_API int          vvr_output_submit(vvr_context* ctx, const vvr_output_request* req);
/* Many regions of one picture as a batch in one request: the tiles of a frame for a detector, fixed-size crops around detections, the crops of
 * test-time augmentation.  One request, one ticket, one ring entry, and one launch per stage whatever `count` is - the region is the third
 * dimension of the grids of k_rescale, k_output_resample, k_output_resample_h and k_output_rgb.
 *   definition   region i receives exactly the bytes that vvr_output_submit stores for the same `req` with x, y = origin[2 i], origin[2 i + 1]
 *            and with dst[k] advanced by i * batch_stride_bytes[k], under the context state in force when the call is accepted: the colour
 *            description, transform, 3-D LUT, normalisation and resampling filter.  No other byte of the destination changes.
 *   req      w, h, out_w, out_h, collocated, format, job, slot and blocking mean what they mean for vvr_output_submit; x and y must be 0.  All
 *            regions have the window's size and the output's size: tap tables, coefficients and tile decomposition are the request's, shared
 *            by the regions, which differ in a source origin and a destination offset only.
 *   regions  may overlap in the source, and two may be equal.  The taps see the region's window as the plane, as a single request does:
 *            samples beyond the window are dropped or clamped exactly as vvr_output_submit does it, even where the picture has samples there.
 *   origin   count pairs x, y in luma samples (even in 4:2:0); read before the call returns.
 *   formats  the ten R'G'B' formats: VVR_OUT_RGB8, _RGB16, _RGBF16, _RGBF32, _RGBA8, _BGRA8, _RGB24, _BGR24, _RGB10A2, _RGBA16F.
 *   resampling   none (out_w = out_h = 0 or the window's size), the reference's DCTIF (no filter set) and the three filters of
 *            vvr_set_output_resampling, each in its range.
 *   ticket   one, from the ticket space of vvr_output_submit: vvr_output_test, _wait, _stream_wait and vvr_sync treat it like any other.
 *   dst      pageable host memory, memory of vvr_host_alloc or device memory, by vvr_output_submit's rules applied to the whole batch: plane k
 *            of the batch is the span dst[k] .. dst[k] + ( count - 1 ) * batch_stride_bytes[k] + the plane's extent, and every used plane's
 *            span must lie wholly inside one kind of memory (a span partly inside a device range, and device spans mixed with host spans, are
 *            refused).  On the device k_output_rgb stores a plane of every region itself, with no copy, when the plane's rows are back to back,
 *            dst[k] is aligned to 32 bytes and batch_stride_bytes[k] is a multiple of 32 - a contiguous ( N, 3, H, W ) or ( N, H, W, C ) tensor
 *            at the usual sizes; any other layout goes through the entry's scratch and device-to-device copies.
 *   refused  VVR_ERR_PARAMETER with a text that names vvr_output_submit_batch, before a ring entry is taken: a struct_size that is not the size of
 *            its struct (either one); count 0 or above VVR_OUT_BATCH_MAX; origin NULL; req->x | req->y non-zero; an origin whose window leaves the
 *            picture or is odd in 4:2:0 (the text names the region's index); grain (the seed chain is defined per frame); a format outside the
 *            ten; a batch_stride_bytes[k] of a used plane below that plane's extent ( rows - 1 ) * dst_stride_bytes[k] + row bytes (regions
 *            would overlap in the destination); a batch whose device buffers in the entry - outputs not stored directly, resampled 4:2:0 frames,
 *            horizontal results of the two-launch form - would exceed 512 MiB in total (a stated limit, named in the text); everything
 *            vvr_output_submit refuses for the same req, with its text behind the new name.  VVR_ERR_BUSY and VVR_NOT_READY as vvr_output_submit.
 *   not offered   regions of different sizes in one request (submit one batch per size); the Y'CbCr and planar formats; grain; more than 256
 *            regions; batches for the measures, statistics and hashes. */
#define VVR_OUT_BATCH_MAX 256
typedef struct vvr_output_batch {
  uint32_t       struct_size;            /* sizeof( vvr_output_batch ) */
  uint32_t       count;                  /* 1 .. VVR_OUT_BATCH_MAX */
  const int32_t* origin;                 /* count pairs x, y: luma samples, even in 4:2:0; read before the call returns */
  size_t         batch_stride_bytes[3];  /* region i of plane k starts at (char*) req->dst[k] + i * batch_stride_bytes[k] */
} vvr_output_batch;                      /* 40 bytes */
VVR_API int          vvr_output_submit_batch(vvr_context* ctx, const vvr_output_request* req, const vvr_output_batch* batch);
VVR_API int          vvr_output_test(vvr_context* ctx, int ticket);
VVR_API int          vvr_output_wait(vvr_context* ctx, int ticket);
/* Destinations of the output queue in device memory, for a consumer on the same GPU (an encoder, a torch model, the sender of a collective).
 * vvr_device_alloc: hipMalloc on the context's device, owned by the context (freed by vvr_destroy at the latest); vvr_device_free gives it back
 * (an unknown pointer: nothing is freed, the text says so; a range a request in flight writes is freed behind that request).
 * vvr_device_register: device memory of the caller's (a torch tensor's storage) on the context's device - the caller's word, nothing is
 * queried.  A range that overlaps a known one, a NULL pointer or 0 bytes: VVR_ERR_PARAMETER.  vvr_device_unregister: VVR_ERR_PARAMETER for a
 * pointer that was not registered (memory of vvr_device_alloc is freed, not unregistered), VVR_ERR_BUSY while a request whose ticket has not been
 * retired writes into the range. */
VVR_API void*        vvr_device_alloc(vvr_context* ctx, size_t bytes);
VVR_API void         vvr_device_free(vvr_context* ctx, void* p);
VVR_API int          vvr_device_register(vvr_context* ctx, void* p, size_t bytes);
VVR_API int          vvr_device_unregister(vvr_context* ctx, void* p);
/* the caller's stream (a hipStream_t) waits ON THE DEVICE for the completion of request `ticket` - behind its last kernel or copy; the host does
 * not wait (vvr_stream_wait_job's counterpart for outputs).  For a host destination it means "the copy has landed" (pageable destinations still
 * get their rows in vvr_output_wait).  The ticket stays and is retired by vvr_output_wait as ever.  An unknown or retired ticket:
 * VVR_ERR_PARAMETER; a request whose job had failed when it was submitted: the job's status, nothing is enqueued. */
VVR_API int          vvr_output_stream_wait(vvr_context* ctx, int ticket, void* stream);
/* decoded picture hash of a slot, as the decoded-picture-hash SEI defines it and the reference checks it (calcMD5 / calcCRC / calcChecksum,
 * PicYuvMD5.cpp:99-221): one digest per component over the whole plane in raster order, samples as 1 byte (bit depth 8) or 2 bytes little
 * endian.  digest receives num_components x digest_len bytes (MD5 16, CRC 2, checksum 4), *digest_len the length of one.  CRC and checksum
 * are computed on the device (only per-row partial results cross PCIe); for MD5, a serial chain over the bytes of a plane, the device packs
 * the plane to exactly those bytes and the host hashes them.  Waits for all work of the context (vvr_sync); vvr_hash_submit below does not. */
enum { VVR_HASH_MD5 = 0, VVR_HASH_CRC = 1, VVR_HASH_CHECKSUM = 2 };
VVR_API int          vvr_picture_hash(vvr_context* ctx, int slot, int method, uint8_t* digest, int* digest_len);
/* vvr_picture_hash as a request of the output queue: what a decoder that verifies every picture against its decoded-picture-hash SEI submits
 * next to the picture's output request (the reference: vvdecParams.verifyPictureHash, vvdecPicAttributes.picHashError).  vvr_picture_hash
 * drains the context (vvr_sync); this does not.  Everything said about an output request above holds for a hash request:
 *   ticket and ring   the ticket comes from the same ticket space and the same 8 ring entries as vvr_output_submit's (VVR_ERR_BUSY counts both
 *            kinds); it is collected with vvr_output_test / vvr_output_wait; vvr_output_stream_wait is accepted and means "the digest bytes
 *            (MD5: the picture's bytes) have landed in the context's pinned memory"; vvr_sync waits for it and retires nothing.
 *   ordering the request runs on the context's output stream behind the picture's completion event ON THE DEVICE; pictures submitted after the
 *            ticket was returned that overwrite the slot wait for the request's kernels on the device; submit the request BEFORE the next
 *            picture into the slot.  blocking == 0: VVR_NOT_READY while `job` has not been handed to the device yet - that hand-over is the
 *            only thing vvr_hash_submit ever waits for on the host (no vvr_sync, no device or stream synchronise).  A request for a job
 *            that failed is accepted and fails with the job's status from vvr_output_test / vvr_output_wait.
 *   hashed   exactly what vvr_picture_hash hashes: the picture in the slot at the picture's size (vvr_slot_picture_size), every component
 *            of the context, samples as 1 byte at bit depth 8, else 2 bytes little endian; digest bytes in vvr_picture_hash's order
 *            (num_components x 16 / 2 / 4 bytes).  The film grain's seed chain and the colour description are not touched.
 *   cost     CRC and checksum are finished on the device (one launch over the rows of all planes, one that combines them): 4 bytes per
 *            component cross PCIe and the host does nothing.  MD5 is a serial chain: the device packs the planes to their bytes, the
 *            picture's bytes cross PCIe into pinned memory, vvr_output_test reports VVR_OK once they have landed and vvr_output_wait
 *            hashes them on the calling thread - about one pass of host hashing over the picture per request.
 *   result   vvr_output_wait, when it returns VVR_OK, writes `digest` (unless NULL) and - with `expected`, the SEI's digests in the same
 *            layout, copied inside vvr_hash_submit - *mismatch: bit c set when component c differs, 0 = the picture is verified.
 *            digest and mismatch must stay valid until vvr_output_wait has returned.
 * Refused (VVR_ERR_PARAMETER with a text, no ring entry taken): a struct_size other than sizeof( vvr_hash_request ), no such slot, an unknown
 * method, job < -1, digest and expected both NULL, expected without mismatch. */
typedef struct vvr_hash_request {
  uint32_t struct_size;      /* sizeof( vvr_hash_request ) */
  int32_t  slot;
  int32_t  job;              /* as vvr_output_request.job: >= 0 ordered behind that picture ON THE DEVICE, -1 the slot as submitted work leaves it */
  uint8_t  method;           /* VVR_HASH_MD5 / _CRC / _CHECKSUM */
  uint8_t  blocking;         /* as vvr_output_request.blocking */
  uint8_t  pad[2];
  uint8_t* digest;           /* nc * len bytes (len 16 / 2 / 4), written by vvr_output_wait; may be NULL when `expected` is given */
  const uint8_t* expected;   /* NULL, or nc * len bytes of the SEI's digests: copied inside vvr_hash_submit */
  uint32_t* mismatch;        /* required with `expected`: bit c set when component c differs (what picHashError reports), 0 = verified */
} vvr_hash_request;
VVR_API int          vvr_hash_submit(vvr_context* ctx, const vvr_hash_request* req);
/* Light-level statistics of a picture as a request of the output queue: the per-frame measurements dynamic HDR metadata is made of - what a
 * player that tone-maps by scene (peak detection), a transcoder that writes MaxCLL / MaxFALL (CTA-861.3) or the ST 2094-40 fields (maxscl,
 * average_maxrgb, the maxRGB percentiles) and anything that watches luma histograms would otherwise pull a whole RGB frame over PCIe for.  The
 * reduction runs where the pixels are; 8216 bytes cross PCIe; nothing drains.  The result is integers, defined here to the bit:
 *   window   x, y, w, h in luma samples of the picture in the slot (vvr_slot_picture_size), even in 4:2:0.  Film grain and rescaling are not
 *            offered: content metadata is measured on the decoded picture.  The seed chain is never touched.
 *   hist_y   hist_y[v]: the luma samples of the window, as they lie in the slot, with value v (a slot holds values below 2^bd; a sample above 1023
 *            written from outside counts in bin 1023).  Both modes.
 *   VVR_STATS_RGB   R, G, B of a pixel are the three values of the definition above (VVR_OUT_RGB16) computed at od = bd - the input of the transform
 *            stage: chroma to the luma grid by the 4-tap filter, taps clamped to the WINDOW's chroma, `collocated` of the request, the Q14 matrix of
 *            the colour description that is set when vvr_stats_submit accepts the request (the coefficients travel as kernel arguments: a later
 *            vvr_set_output_colour never changes a request in flight).  hist_maxrgb[v]: pixels with max( R, G, B ) == v.  max_c[c], min_c[c]: the
 *            largest and the smallest value of channel c = R, G, B over the window (max_c: ST 2094-40 maxscl as code values).  The context's
 *            transform, 3-D LUT and normalisation are ignored: the statistics describe the coded signal, not a rendering of it.
 *   VVR_STATS_LUMA  hist_y alone; hist_maxrgb, max_c and min_c are 0.  Works in every context, 4:0:0 included.
 *   bins     at 2^bd and above: 0.  samples = width * height; both histograms sum to it (hist_maxrgb in RGB mode).
 *   ticket and ring, ordering   everything said about a hash request above holds: the ticket comes from the same ticket space and the same 8 ring
 *            entries (VVR_ERR_BUSY counts every kind of request: output, hash, statistics, comparison, SSIM, MS-SSIM); vvr_output_test / vvr_output_wait collect it; vvr_output_stream_wait means
 *            "the words have landed in the context's pinned memory"; vvr_sync waits for it and retires nothing; the request runs on the output
 *            stream behind the picture's completion event ON THE DEVICE (job >= 0) or behind the slot's users (-1); pictures submitted afterwards
 *            that overwrite the slot wait for the request's kernels on the device; blocking == 0: VVR_NOT_READY while `job` has not been handed
 *            to the device; a request for a job that failed is accepted and fails with that job's status, *stats untouched.
 *   result   vvr_output_wait, when it returns VVR_OK, writes *stats: every field, struct_size included.  It must stay valid until then.
 * Refused (VVR_ERR_PARAMETER with a text, no ring entry taken): a struct_size other than sizeof( vvr_stats_request ), no such slot, job < -1, an
 * unknown mode, stats == NULL, a window outside the picture, empty, or odd in a 4:2:0 context, RGB mode in a 4:0:0 context or without a colour
 * description.
 * The intended loop of a player: vvr_stats_submit -> vvr_output_wait -> vvr_light_level -> vvr_output_lut3d_preset( src_peak_nits = the measured
 * pct_nits or max_nits ) -> vvr_set_output_lut3d -> the RGB request of the same picture.  Smoothing over time and scene logic stay with the caller;
 * ST 2094 / CLL SEIs are not parsed here. */
enum { VVR_STATS_LUMA = 0, VVR_STATS_RGB = 1 };
typedef struct vvr_frame_stats {
  uint32_t struct_size;        /* sizeof( vvr_frame_stats ), written with the rest */
  uint32_t mode;               /* VVR_STATS_* of the request */
  uint32_t bit_depth;          /* the context's: bins 0 .. 2^bit_depth - 1 are in use */
  uint32_t pad;
  uint32_t width, height;      /* the window */
  uint64_t samples;            /* width * height */
  uint32_t hist_y[1024];       /* hist_y[v]: luma samples of the window with value v */
  uint32_t hist_maxrgb[1024];  /* RGB mode: pixels with max( R, G, B ) == v */
  uint32_t max_c[3], min_c[3]; /* RGB mode: per channel R, G, B over the window (max_c = ST 2094-40 maxscl as code values) */
} vvr_frame_stats;
typedef struct vvr_stats_request {
  uint32_t struct_size;        /* sizeof( vvr_stats_request ) */
  int32_t  slot;
  int32_t  job;                /* as vvr_output_request.job */
  int32_t  x, y, w, h;         /* window, luma samples (even in 4:2:0) */
  uint8_t  collocated;         /* RGB mode: as vvr_output_request.collocated */
  uint8_t  mode;               /* VVR_STATS_LUMA / VVR_STATS_RGB */
  uint8_t  blocking;           /* as vvr_output_request.blocking */
  uint8_t  pad;
  vvr_frame_stats* stats;      /* written by vvr_output_wait; must stay valid until it has returned */
} vvr_stats_request;
VVR_API int          vvr_stats_submit(vvr_context* ctx, const vvr_stats_request* req);
/* Light levels from RGB-mode statistics; a pure host function, no context, everything in double.  M = 2^bit_depth - 1.
 *   max_code   the highest non-empty bin of hist_maxrgb.
 *   pct_code   the smallest v with cum( v ) * 10000 >= percentile_e4 * samples, cum( v ) = hist_maxrgb[0] + ... + hist_maxrgb[v], in uint64;
 *              percentile_e4 in 1 .. 10000 (9995: 99.95 %).
 *   transfer_characteristics 16 (PQ): with EOTF the ST 2084 EOTF of vvr_output_transform_preset, in cd/m2: max_nits = EOTF( max_code / M ),
 *              pct_nits = EOTF( pct_code / M ), maxscl_nits[c] = EOTF( max_c[c] / M ), avg_nits = ( sum over v, ascending, of hist_maxrgb[v] *
 *              EOTF( v / M ) ) / samples - the frame average of maxRGB, the quantity MaxFALL is the maximum of (max_nits: MaxCLL's).
 *   transfer_characteristics 0: the code fields alone; the nits fields are 0.
 * struct_size, transfer and the pad are set.  Refused (VVR_ERR_PARAMETER, *out untouched): a NULL pointer, statistics whose struct_size is not
 * sizeof( vvr_frame_stats ), whose mode is not VVR_STATS_RGB, whose bit depth is outside 8..10 or whose hist_maxrgb does not sum to `samples`
 * (or samples == 0), a percentile outside 1 .. 10000, any other transfer (HLG is relative: the presets ignore its source peak). */
struct vvr_light_level {       /* (a tag, no typedef: the function has the name) */
  uint32_t struct_size;        /* sizeof( struct vvr_light_level ) */
  uint32_t transfer;           /* the transfer_characteristics the nits fields were computed with, or 0 */
  uint32_t max_code, pct_code;
  double   max_nits, pct_nits, avg_nits;
  double   maxscl_nits[3];
};
VVR_API int          vvr_light_level(const vvr_frame_stats* stats, int transfer_characteristics, uint32_t percentile_e4, struct vvr_light_level* out);
/* A picture compared with a reference frame as a request of the output queue: what a transcoder's quality loop (PSNR against the source, which lies
 * on the same GPU), a conformance check against a .yuv of expected frames (a digest says "differs", not where or by how much) and a parity test
 * would otherwise pull whole planes over PCIe for.  The reduction runs where the pixels are; about a hundred bytes cross PCIe, and one word per
 * block of 64 x 64 luma samples with `map`; nothing drains.  The result is integers, defined here to the bit:
 *   d        ( int32 ) slot sample - ( int32 ) reference sample, both read as unsigned values exactly as they lie: the slot's 16-bit word, the
 *            reference's byte or little-endian 16-bit word.  A reference may hold any value up to 65535; nothing is clipped or masked.  One d * d
 *            reaches 4 294 836 225: every sum is exact in 64 bits for every input.
 *   window   x, y, w, h in luma samples of the picture in the slot (vvr_slot_picture_size), even in 4:2:0; component c of a 4:2:0 context is compared
 *            over ( x >> 1, y >> 1, w >> 1, h >> 1 ) of its plane.  Every component of the context is compared.  The reference planes ARE the window:
 *            their sample ( 0, 0 ) is the window's, ref[c] + j * ref_stride_bytes[c] is row j of component c.  With ref_slot >= 0 the reference is the
 *            same window of the picture in that slot; both pictures must be of the same size.
 *   per component c   samples = width * height; differing: samples with d != 0; sse: the sum of d * d; sad: the sum of |d|; max_abs: the largest |d|;
 *            first_x, first_y: the first differing sample in raster order of the component's window (rows top to bottom, a row left to right), in that
 *            window's coordinates, both 0xffffffff when differing == 0.  The entries of the components a 4:0:0 context lacks are 0 (first: 0xffffffff).
 *   map      NULL, or ceil( w / 64 ) * ceil( h / 64 ) words, row-major: map[by * ceil( w / 64 ) + bx] is the number of differing samples, over all
 *            components, inside the block of 64 x 64 luma samples at ( 64 bx, 64 by ) of the window; a chroma sample ( i, j ) belongs to the block of
 *            ( 2 i, 2 j ).  The map sums to differing[0] + differing[1] + differing[2].
 *   where the reference may lie (ref_slot == -1), as `dst` of an output request:
 *            every plane wholly inside a range of vvr_device_alloc / vvr_device_register: read in place, nothing crosses PCIe; the caller sees to it
 *            that the memory is idle, as for a device destination.  Every plane in memory of vvr_host_alloc: copied to the device straight from it on
 *            the output stream; it must stay untouched until vvr_output_wait has returned.  Any other host memory: copied inside vvr_compare_submit
 *            into the entry's pinned staging, as `expected` of a hash request is: the caller's buffers are free again when the call returns.
 *   ticket and ring, ordering   everything said about a hash or statistics request above holds: the ticket comes from the same ticket space and the
 *            same 8 ring entries (VVR_ERR_BUSY counts all seven kinds of request); vvr_output_test / vvr_output_wait collect it;
 *            vvr_output_stream_wait means "the words have landed in the context's pinned memory"; vvr_sync waits for it and retires nothing; the
 *            request runs on the output stream behind the picture's completion event ON THE DEVICE (job >= 0) or behind the slot's users (-1);
 *            ref_slot is taken as all work submitted so far leaves it (the job == -1 rule, whatever `job` is); the request is a reader of both slots:
 *            a picture submitted afterwards into either waits for the request's first kernel on the device; blocking == 0: VVR_NOT_READY while `job`
 *            (with ref_slot: any picture) has not been handed to the device; a request for a job that failed is accepted and fails with that job's
 *            status, *result and map untouched.  The film grain seed chain and the colour description are not touched.
 *   result   vvr_output_wait, when it returns VVR_OK, writes *result - every field, struct_size included - and map.  Both must stay valid until then.
 * Refused (VVR_ERR_PARAMETER with a text, no ring entry taken): a struct_size other than sizeof( vvr_compare_request ), no such slot or ref_slot,
 * ref_slot == slot, job < -1, result == NULL, a window outside the picture, empty, or odd in a 4:2:0 context, pictures of different sizes in the two
 * slots; without ref_slot: ref_bytes_per_sample other than 1 or 2, a NULL plane among those the context has, a stride below the row, device planes
 * mixed with host planes, a plane partly inside a device range.
 * Not offered here: SSIM, MS-SSIM and XPSNR are requests of their own (vvr_ssim_submit, vvr_msssim_submit, vvr_xpsnr_submit, below); grained frames; results left in device memory.
 * A reference of another size than the window: vvr_set_compare_scaling, below - the window is rescaled to the reference's size; ref_slot is not
 * offered under it, nor is the other direction, a reference scaled to the picture's size. */
typedef struct vvr_frame_compare {
  uint32_t struct_size;            /* sizeof( vvr_frame_compare ), written with the rest */
  uint32_t bit_depth;              /* the context's */
  uint32_t num_components;         /* 1 (4:0:0) or 3 */
  uint32_t pad;
  uint32_t width[3], height[3];    /* the window per component (chroma: >> 1 in 4:2:0) */
  uint64_t samples[3];             /* width * height */
  uint64_t differing[3];           /* samples with d != 0 */
  uint64_t sse[3];                 /* sum of d * d */
  uint64_t sad[3];                 /* sum of |d| */
  uint32_t max_abs[3];             /* largest |d| */
  uint32_t first_x[3], first_y[3]; /* the first differing sample in raster order of the component's window; 0xffffffff both when differing == 0 */
  uint32_t pad2;
} vvr_frame_compare;
typedef struct vvr_compare_request {
  uint32_t struct_size;            /* sizeof( vvr_compare_request ) */
  int32_t  slot;
  int32_t  job;                    /* as vvr_output_request.job */
  int32_t  x, y, w, h;             /* window, luma samples (even in 4:2:0) */
  int32_t  ref_slot;               /* >= 0: the reference is the same window of that slot; -1: ref[] below */
  uint8_t  ref_bytes_per_sample;   /* 1 or 2 (little endian); ignored with ref_slot */
  uint8_t  blocking;               /* as vvr_output_request.blocking */
  uint8_t  pad[2];
  uint32_t pad2;
  const void* ref[3];              /* planes of the WINDOW's size (not the picture's); ref[1], ref[2] unused in 4:0:0 */
  size_t   ref_stride_bytes[3];
  vvr_frame_compare* result;       /* written by vvr_output_wait; must stay valid until it has returned */
  uint32_t* map;                   /* NULL, or ceil( w / 64 ) * ceil( h / 64 ) words, written by vvr_output_wait */
} vvr_compare_request;
VVR_API int          vvr_compare_submit(vvr_context* ctx, const vvr_compare_request* req);
/* PSNR from the sums of a comparison; a pure host function, no context, everything in double.  peak <= 0 means 2^bit_depth - 1 (HM-style callers
 * pass 255 << ( bit_depth - 8 )).  psnr[c] = 10 log10( peak^2 * samples[c] / sse[c] ) for the components that exist, 0 for those that do not;
 * psnr[3]: the same formula from the sums of samples and of sse over the components.  HUGE_VAL where the sse is 0.  Refused (VVR_ERR_PARAMETER, psnr
 * untouched): a NULL pointer, a struct_size other than sizeof( vvr_frame_compare ), a bit depth outside 8..10, samples[0] == 0. */
VVR_API int          vvr_compare_psnr(const vvr_frame_compare* cmp, double peak, double psnr[4]);
/* SSIM of a picture against a reference frame as a request of the output queue: the second number of a transcoder's quality loop.  It is windowed and
 * not linear per window, so it does not follow from the sums of a comparison; it has a kernel of its own and the comparison's plumbing.  The result is
 * integers, defined here to the bit:
 *   samples  L = 2^bit_depth - 1 with the context's bit depth (8 .. 10).  x: the slot's 16-bit word, y: the reference's byte or little-endian 16-bit
 *            word, both read as unsigned values and both clamped: min( value, L ).  (A reference may hold anything up to 65535 and vvr_write_plane can
 *            put anything into a slot: the clamp keeps every intermediate below inside 64 bits.)
 *   window   x, y, w, h, the components' windows ( x >> 1, y >> 1, w >> 1, h >> 1 ) in 4:2:0, the reference planes that ARE the window, ref_slot:
 *            exactly as for vvr_compare_request.
 *   SSIM windows   8 x 8 samples at a stride of 4 in both directions: origins ( 4 i, 4 j ) of the component's window ( w_c x h_c ) for all
 *            4 i + 8 <= w_c and 4 j + 8 <= h_c.  windows_x = w_c >= 8 ? ( w_c - 8 ) / 4 + 1 : 0, windows_y likewise; samples right of or below the
 *            last whole window are not covered; a component narrower or lower than 8 has no windows.
 *   per SSIM window   with N = 64, in int64_t:  s1 = sum x, s2 = sum y, sxx = sum x * x, syy = sum y * y, sxy = sum x * y;
 *            C1 = ( L * L * 4096 + 5000 ) / 10000, C2 = ( 9 * L * L * 4096 + 5000 ) / 10000  (K1 = 0.01, K2 = 0.03 of Wang et al. at N * N: 26634 and
 *            239708 at 8 bits, 428658 and 3857925 at 10);
 *            A1 = 2 * s1 * s2 + C1,  B1 = s1 * s1 + s2 * s2 + C1,
 *            A2 = 2 * ( N * sxy - s1 * s2 ) + C2,  B2 = ( N * sxx - s1 * s1 ) + ( N * syy - s2 * s2 ) + C2,
 *            l = ( A1 << 24 ) / B1,  c = ( A2 * 16777216 ) / B2,  v = ( l * c ) / 16777216; every / is C's division on
 *            int64_t, which truncates toward zero; A2, c and v may be negative.  This is textbook SSIM - uniform 8 x 8 window, population variance
 *            - as a Q24 number: 0 < A1 <= B1 and |A2| <= B2, so |v| <= 2^24; identical windows give exactly 2^24; A1 << 24 and |A2| << 24 stay
 *            below 2^58; | v / 2^24 - the real-valued SSIM with these constants, C1 / N^2 and C2 / N^2 | < 3 * 2^-24.
 *   per component c   width, height: the component's window; windows_x, windows_y; windows = windows_x * windows_y; sum: the sum of v; min: the
 *            smallest v; min_x, min_y: the origin, in samples of the component's window, of the first window in raster order of the window grid that
 *            has that v.  A component without windows has sum 0, min 0x7fffffff, min_x = min_y = 0xffffffff, and so have the two components a
 *            4:0:0 context lacks (their other fields are 0).
 *   map      NULL, or ceil( w / 64 ) * ceil( h / 64 ) words, row-major: the smallest v over the windows of all components whose ORIGIN sample lies in
 *            that block of 64 x 64 luma samples; a chroma origin ( i, j ) belongs to the block of ( 2 i, 2 j ); 0x7fffffff where no origin falls into
 *            the block (a last block 4 samples wide, for one).
 *   where the reference may lie, ticket and ring, ordering, result   everything said for a comparison request above holds (VVR_ERR_BUSY counts all seven
 *            kinds of request); the film grain seed chain and the colour description are not touched.
 * Refused (VVR_ERR_PARAMETER with a text that names vvr_ssim_submit, no ring entry taken): everything vvr_compare_submit refuses, struct_size being
 * sizeof( vvr_ssim_request ), and a window with w < 8 or h < 8.
 * Not offered here: MS-SSIM is a request of its own (vvr_msssim_submit, below).  Not offered: Gaussian windows; grained frames; results left in device memory;
 * under vvr_set_compare_scaling (below: a reference of another size than the window) ref_slot, and a reference scaled to the picture's size. */
typedef struct vvr_frame_ssim {
  uint32_t struct_size;            /* sizeof( vvr_frame_ssim ), written with the rest */
  uint32_t bit_depth;              /* the context's */
  uint32_t num_components;         /* 1 (4:0:0) or 3 */
  uint32_t pad;
  uint32_t width[3], height[3];    /* the window per component (chroma: >> 1 in 4:2:0) */
  uint32_t windows_x[3], windows_y[3];
  uint64_t windows[3];             /* windows_x * windows_y */
  int64_t  sum[3];                 /* sum of v */
  int32_t  min[3];                 /* smallest v; 0x7fffffff without windows */
  uint32_t min_x[3], min_y[3];     /* origin of the first window in raster order that has it; 0xffffffff both without windows */
  uint32_t pad2;
} vvr_frame_ssim;
typedef struct vvr_ssim_request {  /* field by field a vvr_compare_request, but for the types of result and map */
  uint32_t struct_size;            /* sizeof( vvr_ssim_request ) */
  int32_t  slot;
  int32_t  job;                    /* as vvr_output_request.job */
  int32_t  x, y, w, h;             /* window, luma samples (even in 4:2:0), w >= 8 and h >= 8 */
  int32_t  ref_slot;               /* >= 0: the reference is the same window of that slot; -1: ref[] below */
  uint8_t  ref_bytes_per_sample;   /* 1 or 2 (little endian); ignored with ref_slot */
  uint8_t  blocking;               /* as vvr_output_request.blocking */
  uint8_t  pad[2];
  uint32_t pad2;
  const void* ref[3];              /* planes of the WINDOW's size (not the picture's); ref[1], ref[2] unused in 4:0:0 */
  size_t   ref_stride_bytes[3];
  vvr_frame_ssim* result;          /* written by vvr_output_wait; must stay valid until it has returned */
  int32_t* map;                    /* NULL, or ceil( w / 64 ) * ceil( h / 64 ) words, written by vvr_output_wait */
} vvr_ssim_request;
VVR_API int          vvr_ssim_submit(vvr_context* ctx, const vvr_ssim_request* req);
/* mean SSIM from the sums of an SSIM request; a pure host function, no context, in double.  ssim[c] = sum[c] / ( windows[c] * 2^24 ) for the
 * components that have windows, 0 for the others; ssim[3]: the same formula from the sums of `sum` and of `windows` over the components.  Refused
 * (VVR_ERR_PARAMETER, ssim untouched): a NULL pointer, a struct_size other than sizeof( vvr_frame_ssim ), a bit depth outside 8..10,
 * windows[0] == 0. */
VVR_API int          vvr_compare_ssim(const vvr_frame_ssim* s, double ssim[4]);
/* MS-SSIM of a picture against a reference frame as a request of the output queue: the third number of a transcoder's quality loop.  The pyramid
 * is built and every level is reduced on the device; scales x components x 4 words cross PCIe.  Everything not said here is exactly as for
 * vvr_ssim_submit: the window and the components' windows in 4:2:0, the reference planes that ARE the window, ref_slot, where the reference may lie,
 * ticket and ring (VVR_ERR_BUSY counts all seven kinds of request), ordering, the reader of both slots; a failed job fails the request and leaves
 * *result untouched.  The result is integers, defined here to the bit:
 *   level 0  x_0 = min( slot word, L ), y_0 = min( reference byte or little-endian word, L ), L = 2^bit_depth - 1; its size is the component's
 *            window, w_0 x h_0.
 *   level k + 1 from level k, for both images alike: its size is ( w_k >> 1 ) x ( h_k >> 1 ), and the sample ( i, j ) is
 *            ( a( 2 i, 2 j ) + a( 2 i + 1, 2 j ) + a( 2 i, 2 j + 1 ) + a( 2 i + 1, 2 j + 1 ) + 2 ) >> 2: the rounded mean of 2 x 2 samples.  A last odd
 *            column or row is dropped.  The clamp happens once, at level 0, before any averaging; level samples never exceed L.
 *   per level k and component c   SSIM windows of 8 x 8 samples at a stride of 4 over the level's plane: windows_x, windows_y by vvr_ssim_submit's
 *            formula applied to w_k, h_k; per window l, c and v are vvr_ssim_submit's, unchanged - the same C1, C2, N = 64, the same truncating
 *            64-bit divisions, the same bounds on every intermediate.  Reported: width, height (w_k, h_k), windows_x, windows_y,
 *            windows = windows_x * windows_y, sum_cs: the sum of c, the contrast-structure quotient ( A2 * 16777216 ) / B2 in Q24, and sum_v: the
 *            sum of v.  Indices are [level][component]; the entries of levels >= scales and of the components a 4:0:0 context lacks are 0.
 *   Two consequences.  (a) With scales == 1, sum_v[0] and windows[0] equal `sum` and `windows` of a vvr_ssim_submit request of the same window,
 *            exactly.  (b) A sample of a level that lies outside the whole 4 x 4 cells of its plane (column >= 4 * ( w_k / 4 ) or row
 *            >= 4 * ( h_k / 4 )) reaches neither a window of that level nor a window of any deeper level: the windows of a level cover a multiple
 *            of 4 columns that does not exceed w_k, and 8 * ( w_{k+1} / 4 ) <= 4 * ( w_k / 4 ).  (An implementation may build level k + 1 from
 *            whole cells of level k only and leave the never-read last samples of its scratch planes unwritten.)
 * Refused (VVR_ERR_PARAMETER with a text that names vvr_msssim_submit, no ring entry taken): everything vvr_compare_submit refuses, struct_size being
 * sizeof( vvr_msssim_request ); scales outside 1 .. VVR_MSSSIM_MAX_SCALES; a request in which some component of the context has no window at the
 * last level: ( w_c >> ( scales - 1 ) ) < 8 or ( h_c >> ( scales - 1 ) ) < 8, with w_c = w >> 1, h_c = h >> 1 for chroma in 4:2:0.  So five scales need
 * a window of 256 x 256 in 4:2:0 and of 128 x 128 in 4:0:0; a smaller window takes fewer scales.
 * Not offered: a map or a minimum (where a picture is worst is vvr_ssim_submit's answer); Gaussian windows; another pyramid filter than the 2 x 2
 * mean; grained frames; results left in device memory; under vvr_set_compare_scaling (below: a reference of another size than the window)
 * ref_slot, and a reference scaled to the picture's size. */
#define VVR_MSSSIM_MAX_SCALES 5
typedef struct vvr_frame_msssim {
  uint32_t struct_size;            /* sizeof( vvr_frame_msssim ), written with the rest */
  uint32_t bit_depth;              /* the context's */
  uint32_t num_components;         /* 1 (4:0:0) or 3 */
  uint32_t scales;                 /* the request's */
  uint32_t width[VVR_MSSSIM_MAX_SCALES][3], height[VVR_MSSSIM_MAX_SCALES][3];      /* the level's plane per component */
  uint32_t windows_x[VVR_MSSSIM_MAX_SCALES][3], windows_y[VVR_MSSSIM_MAX_SCALES][3];
  uint64_t windows[VVR_MSSSIM_MAX_SCALES][3];      /* windows_x * windows_y */
  int64_t  sum_cs[VVR_MSSSIM_MAX_SCALES][3];       /* sum of c */
  int64_t  sum_v[VVR_MSSSIM_MAX_SCALES][3];        /* sum of v */
} vvr_frame_msssim;                /* 616 bytes */
typedef struct vvr_msssim_request { /* a vvr_ssim_request with `scales` where pad[0] was, and no map */
  uint32_t struct_size;            /* sizeof( vvr_msssim_request ) */
  int32_t  slot;
  int32_t  job;                    /* as vvr_output_request.job */
  int32_t  x, y, w, h;             /* window, luma samples (even in 4:2:0) */
  int32_t  ref_slot;               /* >= 0: the reference is the same window of that slot; -1: ref[] below */
  uint8_t  ref_bytes_per_sample;   /* 1 or 2 (little endian); ignored with ref_slot */
  uint8_t  blocking;               /* as vvr_output_request.blocking */
  uint8_t  scales;                 /* 1 .. VVR_MSSSIM_MAX_SCALES */
  uint8_t  pad;
  uint32_t pad2;
  const void* ref[3];              /* planes of the WINDOW's size (not the picture's); ref[1], ref[2] unused in 4:0:0 */
  size_t   ref_stride_bytes[3];
  vvr_frame_msssim* result;        /* written by vvr_output_wait; must stay valid until it has returned */
} vvr_msssim_request;              /* 96 bytes */
VVR_API int          vvr_msssim_submit(vvr_context* ctx, const vvr_msssim_request* req);
/* MS-SSIM from the sums of an MS-SSIM request; a pure host function, no context, in double.  Per component c: m_k = sum_cs[k][c] /
 * ( windows[k][c] * 2^24 ) for k < scales - 1, m_last = sum_v[scales - 1][c] / ( windows[scales - 1][c] * 2^24 ); msssim[c] = the product over k, in
 * ascending order, of pow( max( m_k, 0 ), weights[k] ).  msssim[3]: the same formula on sum_cs, sum_v and windows summed over the components, per
 * level.  Components that do not exist (or, in sums built by hand, lack windows at one of the levels) give 0.  weights == NULL: the first `scales` of 0.0448, 0.2856, 0.3001, 0.2363, 0.1333 (Wang et al. 2003)
 * divided by their sum; a caller's weights are used as given, `scales` of them.  Refused (VVR_ERR_PARAMETER, msssim untouched): a NULL s or msssim,
 * a struct_size other than sizeof( vvr_frame_msssim ), a bit depth outside 8..10, scales outside 1 .. 5, windows[k][0] == 0 for some k < scales,
 * a weight that is negative or not finite. */
VVR_API int          vvr_compare_msssim(const vvr_frame_msssim* s, const double* weights, double msssim[4]);
/* XPSNR of a picture against a reference frame as a request of the output queue: the number the VVC tool chain itself reports (Helmrich et al.,
 * "XPSNR: a low-complexity extension of PSNR", 2020), a block-wise weighted SSE whose weights come from a spatial high-pass stencil on the reference
 * luma and a temporal difference against the one or two reference frames before it.  It follows from nothing a comparison returns - that has the
 * SSE per frame, not per block, and takes one reference frame - so it has a kernel of its own (k_output_xpsnr) and the comparison's plumbing.  This
 * text follows the structure of XPSNR and is the normative definition; agreement with another implementation's decimals is neither claimed nor
 * tested.  The result is integers, defined here to the bit:
 *   samples  x: the slot's 16-bit word; o: the reference's byte or little-endian word; o1, o2: the previous and the one-before-previous reference
 *            LUMA.  All are read as the unsigned values they are; nothing is clipped or masked, a reference may hold anything up to 65535.
 *   window   x, y, w, h, the components' windows in 4:2:0, the reference planes that ARE the window, ref_slot: exactly as for vvr_compare_request.
 *            prev[0] / prev[1] (o1 / o2; the first `temporal` are used) are luma planes of the window's size, with the same ref_bytes_per_sample and
 *            strides of their own; they are always the caller's memory, also with ref_slot >= 0.  Every plane passed by pointer (ref[] when
 *            ref_slot == -1, and prev[]) lies in one kind of home: all wholly inside device ranges, or all on the host; the three cases are those
 *            of vvr_compare_submit: read in place, copied from vvr_host_alloc memory on the output stream, or staged inside the call.
 *   blocks   B = the request's `block`; for block == 0, B = max( 4, 4 * (int)( 32.0 * sqrt( w * h / 8294400.0 ) + 0.5 ) ) in double: 128 at
 *            3840 x 2160, 64 at 1920 x 1080, 44 at 1280 x 720, 256 at 8K, 8 at 256 x 128, 4 at 208 x 80.  Block ( bx, by ) covers luma
 *            [ B bx, min( B bx + B, w ) ) x [ B by, min( B by + B, h ) ) of the window and, in 4:2:0, the chroma samples ( i, j ) with ( 2 i, 2 j )
 *            inside it.  blocks_x = ceil( w / B ), blocks_y = ceil( h / B ); records are stored row-major.  vvr_xpsnr_blocks gives this geometry.
 *   filter   filter == 0 resolves to 2 when w * h > 2048 * 1152, else to 1.
 *            Filter 1, positions ( i, j ) of the luma window with 1 <= i <= w - 2 and 1 <= j <= h - 2:
 *              f = 12 o(i,j) - 2 [ o(i-1,j) + o(i+1,j) + o(i,j-1) + o(i,j+1) ] - [ o(i-1,j-1) + o(i+1,j-1) + o(i-1,j+1) + o(i+1,j+1) ];
 *              t = 0 (temporal 0), | o - o1 | (temporal 1), | o - 2 o1 + o2 | (temporal 2), at ( i, j ).
 *            Filter 2, the same shape on 2 x 2 sums, positions ( i, j ) with i and j even, 2 <= i <= w - 4, 2 <= j <= h - 4: f is the sum over
 *            di, dj = 0 .. 5 of W[dj][di] * o( i - 2 + di, j - 2 + dj ) with the symmetric weights (their sum is 0)
 *                 0 -1 -1 -1 -1  0
 *                -1 -2 -3 -3 -2 -1
 *                -1 -3 12 12 -3 -1
 *                -1 -3 12 12 -3 -1
 *                -1 -2 -3 -3 -2 -1
 *                 0 -1 -1 -1 -1  0
 *              and with S(a) = a(i,j) + a(i+1,j) + a(i,j+1) + a(i+1,j+1):  t = 0, | S(o) - S(o1) |, | S(o) - 2 S(o1) + S(o2) |.
 *            A position belongs to the block that contains ( i, j ); B is a multiple of 4, so a 2 x 2 cell never straddles blocks.
 *            |f| <= 48 * 65535 < 2^22 and t <= 2^20: every sum is exact in 64 bits for every input (a 32-bit sum over 64 x 64 samples is not, for
 *            references above the bit depth).
 *   per block (vvr_xpsnr_block)   sse[c]: the sum of ( x - o )^2 over the block's samples of component c, the d of vvr_compare_submit;
 *            act_spatial: the sum of |f|, act_temporal: the sum of t, count: the number of positions, all over the block's positions; pad = 0.  The
 *            entries of the components a 4:0:0 context lacks are 0.
 *   per frame (vvr_frame_xpsnr)   struct_size, bit_depth, num_components, temporal, filter (resolved: 1 or 2), block (resolved), blocks_x, blocks_y,
 *            width, height, samples per component, and sse[3], act_spatial, act_temporal, count: the sums over the blocks.
 *   Three consequences.  (a) sse[c] equals vvr_compare_submit's for the same request.  (b) The frame's sums do not depend on B.  (c) act_spatial,
 *            act_temporal and count do not depend on the slot.
 *   ticket and ring, ordering, result   everything said for a comparison request above holds (VVR_ERR_BUSY counts all seven kinds of request); the
 *            request is a reader of both slots; a request for a job that failed fails with that job's status, *result and blocks untouched.
 *            vvr_output_wait, when it returns VVR_OK, writes *result and, unless `blocks` is NULL, blocks_x * blocks_y records.
 * Refused (VVR_ERR_PARAMETER with a text that names vvr_xpsnr_submit, no ring entry taken): everything vvr_compare_submit refuses, struct_size being
 * sizeof( vvr_xpsnr_request ); w < 8 or h < 8; temporal > 2; filter > 2; a block that is neither 0 nor a multiple of 4; more than 16384 blocks; for
 * k < temporal a NULL prev[k] or a stride below the row; a prev plane partly inside a device range; pointer planes of mixed homes.
 * Not offered: minimum-smoothing of the weights between neighbouring blocks at low resolutions; chroma activity; temporal activity from slots;
 * grained frames; results left in device memory; more than 16384 blocks; under vvr_set_compare_scaling (below: a reference of another size than
 * the window) ref_slot, and a reference scaled to the picture's size. */
#define VVR_XPSNR_MAX_BLOCKS 16384
typedef struct vvr_xpsnr_block {
  uint64_t sse[3];                 /* sum of ( x - o )^2 per component */
  uint64_t act_spatial;            /* sum of |f| */
  uint64_t act_temporal;           /* sum of t */
  uint32_t count;                  /* positions in the block */
  uint32_t pad;                    /* 0 */
} vvr_xpsnr_block;                 /* 48 bytes */
typedef struct vvr_frame_xpsnr {
  uint32_t struct_size;            /* sizeof( vvr_frame_xpsnr ), written with the rest */
  uint32_t bit_depth;              /* the context's */
  uint32_t num_components;         /* 1 (4:0:0) or 3 */
  uint32_t temporal;               /* the request's */
  uint32_t filter;                 /* resolved: 1 or 2 */
  uint32_t block;                  /* resolved: B */
  uint32_t blocks_x, blocks_y;
  uint32_t width[3], height[3];    /* the window per component (chroma: >> 1 in 4:2:0) */
  uint64_t samples[3];             /* width * height */
  uint64_t sse[3];                 /* the sums over the blocks */
  uint64_t act_spatial, act_temporal, count;
} vvr_frame_xpsnr;                 /* 128 bytes */
typedef struct vvr_xpsnr_request {
  uint32_t struct_size;            /* sizeof( vvr_xpsnr_request ) */
  int32_t  slot;
  int32_t  job;                    /* as vvr_output_request.job */
  int32_t  x, y, w, h;             /* window, luma samples (even in 4:2:0), w >= 8 and h >= 8 */
  int32_t  ref_slot;               /* >= 0: the reference is the same window of that slot; -1: ref[] below */
  uint8_t  ref_bytes_per_sample;   /* 1 or 2 (little endian), of ref[] and prev[]; ignored with ref_slot: prev[] holds 16-bit words then */
  uint8_t  blocking;               /* as vvr_output_request.blocking */
  uint8_t  temporal;               /* 0, 1, 2: how many of prev[] are used */
  uint8_t  filter;                 /* 0: by the window's size; 1, 2 */
  uint32_t block;                  /* 0: by the formula; else a multiple of 4 */
  const void* ref[3];              /* planes of the WINDOW's size (not the picture's); ref[1], ref[2] unused in 4:0:0 */
  size_t   ref_stride_bytes[3];
  const void* prev[2];             /* luma of the reference one and two frames earlier, of the window's size; the first `temporal` are used */
  size_t   prev_stride_bytes[2];
  vvr_frame_xpsnr* result;         /* written by vvr_output_wait; must stay valid until it has returned */
  vvr_xpsnr_block* blocks;         /* NULL (totals only), or blocks_x * blocks_y records, written by vvr_output_wait */
} vvr_xpsnr_request;               /* 136 bytes */
VVR_API int          vvr_xpsnr_submit(vvr_context* ctx, const vvr_xpsnr_request* req);
/* the geometry a caller sizes `blocks` with: B, blocks_x and blocks_y of a window of w x h with the request's `block`, by the words above.  A pure
 * host function.  Refused (VVR_ERR_PARAMETER, outputs untouched): a NULL pointer, w < 8 or h < 8, a block that is neither 0 nor a multiple of 4,
 * more than 16384 blocks. */
VVR_API int          vvr_xpsnr_blocks(int w, int h, uint32_t block, uint32_t* resolved_block, uint32_t* blocks_x, uint32_t* blocks_y);
/* XPSNR from the records of an XPSNR request; a pure host function, no context, everything in double, the blocks in ascending order.  Per block k:
 * q_k = count_k * ( filter == 2 ? 4 : 1 );  act_k = count_k ? 1 + act_spatial_k / q_k + 2 * act_temporal_k / q_k : 0;  act_k = max( act_k,
 * 2^( bit_depth - 6 ) );  w_k = sqrt( a_pic ) / act_k, a_pic <= 0 meaning 2^( 2 * bit_depth - 9 ) * sqrt( 3840.0 * 2160.0 / ( width[0] *
 * height[0] ) ).  wsse_c = the sum over k of w_k * sse_k[c];  xpsnr[c] = 10 log10( peak^2 * samples[c] / wsse_c ), peak <= 0 meaning
 * 2^bit_depth - 1;  xpsnr[3]: the same formula from the sums of wsse and of samples over the components, as vvr_compare_psnr does.  HUGE_VAL where
 * wsse is 0; 0 for components that do not exist.  a_pic scales all weights of a frame alike: a caller who matches another tool's normalisation
 * passes its constant.  Refused (VVR_ERR_PARAMETER, xpsnr untouched): a NULL pointer, a struct_size other than sizeof( vvr_frame_xpsnr ), a bit
 * depth outside 8..10, samples[0] == 0, blocks_x * blocks_y == 0, filter outside 1..2. */
VVR_API int          vvr_compare_xpsnr(const vvr_frame_xpsnr* f, const vvr_xpsnr_block* blocks, double a_pic, double peak, double xpsnr[4]);
/* A reference of another size than the window, for the four measures above - vvr_compare_submit, vvr_ssim_submit, vvr_msssim_submit,
 * vvr_xpsnr_submit: the rungs of an adaptive-bitrate ladder below the top one are coded at a reduced size and judged after upscaling to the
 * source's, and a stream with reference picture resampling changes its picture size mid-sequence while its source does not.  Context state like
 * the narrowing (vvr_set_output_narrowing): a new context has ( 0, 0 ) - scaling off, every request means what is said above - and the value is
 * read once, under the context's mutex, when a request is submitted; a request in flight keeps the value it was submitted with.  The request
 * structs do not change.  out_w, out_h: luma samples; collocated: as vvr_read_output_scaled takes it (bit 0: chroma collocated horizontally,
 * bit 1: vertically; luma is always collocated).
 * With scaling on, a request of the four kinds submitted from then on is defined to the bit:
 *   picture side   component c of the window - x, y, w, h of the request, validated against the picture in the slot as before - rescaled to
 *            ( out_w >> s ) x ( out_h >> s ), s = 1 for the chroma of a 4:2:0 context: exactly the samples vvr_read_output_scaled delivers for that
 *            component, that window of its plane, that size and `collocated` with bytes_per_sample == 2.  out_w == w && out_h == h is not special.
 *   everything downstream of the window   takes out_w x out_h where it took w x h: the reference planes ARE the rescaled window - their rows,
 *            extents, staging and device-range checks are those of planes of that size; width[], height[], samples[] and windows*[] of the
 *            results; the blocks of 64 x 64 luma samples of the maps, ceil( out_w / 64 ) * ceil( out_h / 64 ) of them; the 8 x 8 minimum of SSIM and
 *            XPSNR; the last-level condition of MS-SSIM; XPSNR's block formula, default filter, block count limit (vvr_xpsnr_blocks( out_w, out_h,
 *            ... )) and prev[] planes; first_x, first_y and min_x, min_y are coordinates of the rescaled window.
 *   refused at submit (VVR_ERR_PARAMETER, a text that names the submitting function, no ring entry taken), besides all that is refused without
 *            scaling: out_w outside [ceil( w / 8 ), 8 w] or out_h outside [ceil( h / 8 ), 8 h] - the rule of vvr_read_output_scaled; ref_slot >= 0.
 * An SSIM, MS-SSIM or XPSNR request keeps the rescaled planes in its ring entry on the device and stops being a reader of the slot when they
 * are written: a picture submitted afterwards into the slot waits for the rescaling, not for the measure.  A comparison request rescales and
 * compares in one kernel and stores no rescaled sample; its words are those of the comparison of the rescaled planes.  The film grain seed
 * chain and the colour description are not touched.
 * Refused (VVR_ERR_PARAMETER, the text names vvr_set_compare_scaling, the value set before stays in force): exactly one of the two sides 0; a
 * side outside 1 .. 8192; an odd side in a 4:2:0 context; collocated outside 0 .. 3.
 * Not offered: grained frames; ref_slot under scaling (two slots of different picture sizes); the other direction, a reference scaled to the
 * picture's size; results left in device memory. */
VVR_API int          vvr_set_compare_scaling(vvr_context* ctx, int out_w, int out_h, int collocated);
/* the finished picture in `slot` (every plane, at the picture's size) into the caller's buffers - what a decoder does with each picture it hands to
 * the application (the planes of a vvdecFrame live in the Picture's own buffers, vvdecimpl.cpp:1058).  Waits for NOTHING: the caller has waited for
 * the picture (vvr_wait); other pictures in flight are not held up (vvr_read_plane drains the context).  Each plane crosses PCIe in one transfer
 * into pinned memory of the context, from where `threads` (1..16) threads lay the rows out at dst[c] with dst_stride_samples[c]: a copy straight
 * into pageable memory runs at a fraction of the link's rate.  May be called by several threads at once (one staging buffer per call in flight). */
VVR_API int          vvr_read_picture(vvr_context* ctx, int slot, uint16_t* const* dst, const size_t* dst_stride_samples, int threads);
/* upload a reference picture produced elsewhere (another GPU / a test) into a slot */
VVR_API int          vvr_write_plane(vvr_context* ctx, int slot, int comp, const uint16_t* src, size_t src_stride_samples);
/* size of the picture a slot holds (luma samples; a picture lies in the top left corner of its slot): vvr_submit sets it to the size of the picture
 * it reconstructs into the slot, this call is for pictures that come from outside (vvr_write_plane) when they are smaller than the context's
 * pictures - a coded video sequence with reference picture resampling.  vvr_read_plane, vvr_write_plane and vvr_picture_hash move / cover that
 * many samples; a new context's slots have the context's size.                                                                              */
VVR_API int          vvr_slot_picture_size(vvr_context* ctx, int slot, int width, int height);
/* DMVR refined delta MVs of job (TaskFinishMotionInfo, DecCu.cpp:161): copies num_entries * 2 int32 */
VVR_API int          vvr_read_dmvr(vvr_context* ctx, int job, int32_t* dst, size_t num_entries);
/* Collocated motion of a picture submitted with VVR_TOOL_COL_MOTION (blocks until the job is done): ceil(w4 / 2) * ceil(h4 / 2) records in raster order,
 * record (x, y) = the final motion of the 4x4 unit (2x, 2y) - the layout of ColocatedMotionInfo = MotionInfo (MotionInfo.h:157), what
 * DecCu::TaskFinishMotionInfo leaves in CtuData::colMotion.  Returns the number of records of the picture (copies at most num_entries), < 0 on error. */
VVR_API int          vvr_read_col_motion(vvr_context* ctx, int job, vvr_motion* dst, size_t num_entries);
/* Two-step submission, for measurements of the device pipeline alone (bench.py's device_only_fps) and for pictures that are reconstructed more
 * than once: vvr_prepare validates the description, runs the host glue (builds the device work lists the reference iterates over in
 * DecCu::TaskTrafoCtu / TaskInterCtu, DecCu.cpp:106-134) and makes everything resident in HBM - it allocates device memory of the picture's
 * size and copies through pinned staging of the context with a blocking call, i.e. it is a set-up call, not part of a pipeline; vvr_submit_prepared only enqueues kernels.
 * A host that streams pictures uses vvr_submit with vvr_config.host_threads > 0: the same steps on the library's worker threads and upload ring,
 * without an allocation per picture. */
typedef struct vvr_prepared vvr_prepared;
VVR_API int          vvr_prepare(vvr_context* ctx, const vvr_picture* host_pic, vvr_prepared** out);
VVR_API int          vvr_submit_prepared(vvr_context* ctx, vvr_prepared* prepared);
VVR_API void         vvr_free_prepared(vvr_context* ctx, vvr_prepared* prepared);
/* the HIP stream (hipStream_t) job `job` runs on, and the per-kernel timing of the last waited job (bench/profiling) */
VVR_API void*        vvr_job_stream(vvr_context* ctx, int job);
/* External producers and consumers of DPB slots - the collective that replicates a reference picture to the GPUs whose pictures predict from it
 *  - ordered on the DEVICE: the host never waits for a picture.
 *   vvr_stream_wait_job   `stream` (hipStream_t of the caller) waits for picture `job`: what a sender does before the collective reads the slot;
 *   vvr_stream_wait_slot  `stream` waits for every picture submitted so far that reads or writes `slot` (and for earlier external users): what a
 *                         receiver does before the collective overwrites the slot;
 *   vvr_slot_external_event  pictures submitted from now on that use `slot` wait for `event` (hipEvent_t, recorded by the caller behind its
 *                         collective) first; writes != 0: the external work wrote the slot (earlier users were ordered before it by
 *                         vvr_stream_wait_slot), 0: it only reads it (a sender: later pictures must not overwrite the slot under it).  The
 *                         back-end keeps the handle until the slot is next written (by a picture or by an external writer) or until
 *                         vvr_sync finds the event complete - nowhere else does it look: the caller keeps the event alive until it is
 *                         complete AND a vvr_sync has returned since (or the slot has been overwritten).  The event should be recorded
 *                         before it is registered: one that is recorded later is still waited for by every picture handed to the device
 *                         after the record, but a vvr_sync in between forgets it (an event that was never recorded reads as complete).
 * A picture can only be waited for once it has been handed to the device (its work lists are built by worker threads): blocking = 0 returns
 * VVR_NOT_READY instead of waiting for that on the host.                                                                                      */
VVR_API int          vvr_stream_wait_job(vvr_context* ctx, int job, void* stream, int blocking);
VVR_API int          vvr_stream_wait_slot(vvr_context* ctx, int slot, void* stream, int blocking);
VVR_API int          vvr_slot_external_event(vvr_context* ctx, int slot, void* event, int writes);
VVR_API const char*  vvr_last_error(const vvr_context* ctx);
VVR_API const char*  vvr_version(void);
/* sizeof() of ABI struct number `which` as this library was compiled (0 vvr_pic_header, 1 vvr_cu, 2 vvr_tu, 3 vvr_motion,
 * 4 vvr_lfp, 5 vvr_sao_ctu, 6 vvr_alf_ctu, 7 vvr_alf_params, 8 vvr_lmcs_params, 9 vvr_picture, 10 vvr_config,
 * 11 vvr_kernel_stat, 12 vvr_wp_params, 13 vvr_scaling_list, 14 vvr_subpic, 15 vvr_slice_header; anything else 0): lets a binding written in another language verify its struct mirror at load time */
VVR_API size_t       vvr_abi_sizeof(int which);

/* kernel statistics accumulated with HIP events on the launch streams when enabled */
typedef struct vvr_kernel_stat {
  char     name[32];
  uint64_t launches;
  double   total_ms;
  double   algo_bytes;           /* algorithmic bytes moved by these launches (SURVEY.md §8(d) model) */
} vvr_kernel_stat;
VVR_API int          vvr_enable_stats(vvr_context* ctx, int on);
VVR_API int          vvr_get_stats(vvr_context* ctx, vvr_kernel_stat* out, int max_entries);
/* practical HBM ceiling of this device: bytes per second (read + written) of the library's device copy kernel over as much of the DPB
 * as the context's scratch planes hold (hundreds of MB for a 4K context: far beyond the caches), HIP-event timed, averaged over `iters` launches;
 * the DPB is only read, the scratch planes hold nothing between pictures */
VVR_API double       vvr_measure_copy_bandwidth(vvr_context* ctx, int iters);

/* Host glue helpers (pure functions, no device): what the reference computes per CU/TU on the CPU before the
 * arithmetic starts.  They are part of the ABI so that the parser-side integration and the tests use one definition. */
/* TrQuant::getTrTypes (TrQuant.cpp:330) -> (ver<<2)|hor */
VVR_API uint8_t      vvr_resolve_tr_type(const vvr_pic_header* hdr, const vvr_cu* cu, const vvr_tu* tu, int comp, int implicit_mts, int explicit_mts_intra, int explicit_mts_inter);

#ifdef __cplusplus
}
#endif
#endif /* VVR_H */
