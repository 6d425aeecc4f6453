// TEST INFRASTRUCTURE (tests/ only): what k_itrans (vvdec_amd/csrc/vvr_kernels.hip) rests on since its passes run on packed 16-bit pairs, checked on the CPU.
//   1. tb_record (vvr_device.h, compiled here as it is for the device): the 16-byte record of a transform block against the chase it replaces - item -> TU record
//      -> CU record, the LFNST set from the reference's table (vvc_lfnst_lut) and the wide-angle mapping with its table of shifts - for every coded block of
//      the pictures whose CU / TU arrays the files named on the command line hold (written by tests/test_itrans_replay.py), with every mode / ICT / slice-bit value.
//   2. the pair indexing of both passes: threads as loops, LDS as arrays of exactly the kernel's sizes (the sanitizer sees an index that leaves them), filled with
//      garbage before every block; levels stored as pairs of rows, basis rows staged as pairs with the upper half of an odd last pair zero, v_dot2_i32_i16 as two
//      products and an add in 64 bits (the sum must fit 32), pass 1 writing its four columns as two pairs, the scalar forms (2-wide blocks, 2-high blocks, 1-D
//      blocks) reading the same layout - against the plain triple loop, for every block size of the three classes, every transform type and every count of rows /
//      columns that take part (odd ones included), with operands at the ends of the 16-bit range.
// It restates the kernel's loops, it does not compile them: a change to the kernel has to be made here as well.  Prints "all equal" and returns 0.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <algorithm>
#include "../vvdec_amd/csrc/vvr_device.h"
#include "../tables/vvc_tables.inc"

static int failures = 0;
#define CHECK( c, ... ) do { if( !( c ) ) { if( failures++ < 20 ) { printf( "FAILED %s: ", #c ); printf( __VA_ARGS__ ); printf( "\n" ); } } } while( 0 )

// ---------------------------------------------------------------------------------------------------------------------------------------------------------
// 1. the record
// ---------------------------------------------------------------------------------------------------------------------------------------------------------
static int ilog2i( int v ) { int l = 0; while( v > 1 ) { v >>= 1; l++; } return l; }
static int wideAngle( int w, int h, int mode )      // PU::getWideAngIntraMode
{
  static const int modeShift[6] = { 0, 6, 10, 12, 14, 15 };
  if( mode < 2 ) return mode;
  const int d = abs( ilog2i( w ) - ilog2i( h ) );
  if( w > h && mode < 2 + modeShift[d] ) mode += 65;
  else if( h > w && mode > 66 - modeShift[d] ) mode -= 67;
  return mode;
}

static size_t checkRecords( const char* path )
{
  FILE* f = fopen( path, "rb" );
  if( !f ) { printf( "cannot open %s\n", path ); failures++; return 0; }
  uint32_t hd[4];
  if( fread( hd, 4, 4, f ) != 4 || hd[0] != sizeof( vvr_cu ) || hd[1] != sizeof( vvr_tu ) ) { printf( "%s: header / record sizes\n", path ); failures++; fclose( f ); return 0; }
  std::vector<vvr_cu> cus( hd[2] ); std::vector<vvr_tu> tus( hd[3] );
  if( fread( cus.data(), sizeof( vvr_cu ), cus.size(), f ) != cus.size() || fread( tus.data(), sizeof( vvr_tu ), tus.size(), f ) != tus.size() ) { printf( "%s: short file\n", path ); failures++; fclose( f ); return 0; }
  fclose( f );
  size_t blocks = 0;
  for( size_t t = 0; t < tus.size(); t++ )
  {
    const vvr_tu& tu = tus[t];
    if( tu.cu >= cus.size() ) { failures++; continue; }
    const vvr_cu& cu = cus[tu.cu];
    for( int comp = 0; comp < 3; comp++ )
    {
      if( !( tu.comp_mask & ( 1 << comp ) ) || !( cu.flags & VVR_CU_ROOT_CBF ) ) continue;
      // (joint Cb-Cr: the levels belong to Cb for modes 2 / 3, to Cr for mode 1)
      if( comp && tu.joint_cbcr ) { if( comp != ( ( tu.joint_cbcr >> 1 ) ? 1 : 2 ) ) continue; }
      else if( !( tu.cbf & ( 1 << comp ) ) ) continue;
      // the item as PrepScratch::buildWorkLists forms it (mode and ict: every value)
      TbItem it; it.tu = (uint32_t) t; it.comp = (uint8_t) comp;
      it.pad = (uint8_t) ( ( ( comp && cu.isp_mode ) ? TB_P_CUGEOM : 0 ) | ( ( comp ? cu.bdpcm[1] : cu.bdpcm[0] ) ? TB_P_BDPCM : 0 ) | ( ( cu.lfnst_idx && ( cu.tree != VVR_TREE_JOINT || comp == 0 ) ) ? TB_P_LFNST : 0 ) );
      // the chase of the kernel before the record
      const int csh = comp ? 1 : 0;
      int bw = tu.w >> csh, bh = tu.h >> csh, bx = tu.x >> csh, by = tu.y >> csh;
      if( it.pad & TB_P_CUGEOM ) { bw = cu.w >> 1; bh = cu.h >> 1; bx = cu.x >> 1; by = cu.y >> 1; }
      if( bw < 1 || bh < 1 ) continue;
      int set = 0, idx = 0; bool transpose = false;
      if( it.pad & TB_P_LFNST )
      {
        int mode;
        if( ( cu.flags & VVR_CU_MIP ) && comp == 0 ) mode = 0;
        else if( comp && cu.intra_dir[1] >= 67 ) mode = cu.lfnst_intra_mode;
        else mode = cu.intra_dir[comp ? 1 : 0];
        mode = wideAngle( ( cu.isp_mode && !comp ) ? cu.w : bw, ( cu.isp_mode && !comp ) ? cu.h : bh, mode );
        const int lm = mode < 0 ? mode + 14 + 67 : mode >= 67 ? mode + 14 : mode;
        transpose = ( lm >= 67 && lm >= 67 + 14 ) || ( lm < 67 && lm > 34 );
        CHECK( lm >= 0 && lm < 97, "LFNST mode %d", lm );
        set = vvc_lfnst_lut[std::min( std::max( lm, 0 ), 96 )]; idx = cu.lfnst_idx - 1;
      }
      for( int v = 0; v < 64; v++ )
      {
        it.mode = (uint8_t) ( v & 1 ); it.ict = (uint8_t) ( ( v >> 1 ) & 7 );
        const uint32_t sliceFlags = ( ( v >> 4 ) & 1 ? VVR_TOOL_DEP_QUANT : 0 ) | ( ( v >> 5 ) & 1 ? VVR_TOOL_SCALING_LIST : 0 ) | VVR_TOOL_LFNST | VVR_TOOL_MTS;
        const TbRec r = tb_record( it, tu, cu, sliceFlags );
        CHECK( sizeof( TbRec ) == 16, "record size" );
        CHECK( ( 1 << tbr_lw( r ) ) == bw && ( 1 << tbr_lh( r ) ) == bh && r.x == bx && r.y == by, "geometry of TU %zu comp %d: %dx%d at %d,%d, record %dx%d at %d,%d", t, comp, bw, bh, bx, by, 1 << tbr_lw( r ), 1 << tbr_lh( r ), r.x, r.y );
        CHECK( tbr_comp( r ) == comp && tbr_mode( r ) == it.mode && tbr_ict( r ) == it.ict, "comp / mode / ict of TU %zu comp %d", t, comp );
        CHECK( r.coef == tu.coef_off[comp] && tbr_scan_x( r ) == tu.max_scan_x[comp] && tbr_scan_y( r ) == tu.max_scan_y[comp] && tbr_qp( r ) == tu.qp[comp], "levels / QP of TU %zu comp %d", t, comp );
        CHECK( tbr_mts( r ) == tu.mts_idx[comp] && tbr_tr_type( r ) == tu.tr_type[comp], "transform of TU %zu comp %d", t, comp );
        CHECK( tbr_bdpcm( r ) == ( comp ? cu.bdpcm[1] : cu.bdpcm[0] ), "BDPCM of TU %zu comp %d", t, comp );
        CHECK( tbr_dep_quant( r ) == ( ( v >> 4 ) & 1 ) && tbr_sl_on( r ) == ( ( v >> 5 ) & 1 ), "slice bits of TU %zu comp %d", t, comp );
        CHECK( tbr_list_type( r ) == ( cu.pred_mode == VVR_PRED_INTRA ? 0 : 3 ) + comp, "scaling-list type of TU %zu comp %d", t, comp );
        CHECK( tbr_lfnst( r ) == ( ( it.pad & TB_P_LFNST ) != 0 ), "LFNST bit of TU %zu comp %d", t, comp );
        if( it.pad & TB_P_LFNST ) CHECK( tbr_lfnst_set( r ) == set && tbr_lfnst_idx( r ) == idx && tbr_lfnst_transposed( r ) == transpose, "LFNST set / index / transposition of TU %zu comp %d", t, comp );
      }
      blocks++;
    }
  }
  return blocks;
}

// ---------------------------------------------------------------------------------------------------------------------------------------------------------
// 2. the packed passes
// ---------------------------------------------------------------------------------------------------------------------------------------------------------
static const int16_t* trMatrix( int type, int n )
{
  if( type == 0 ) { switch( n ) { case 2: return vvc_dct2_2; case 4: return vvc_dct2_4; case 8: return vvc_dct2_8; case 16: return vvc_dct2_16; case 32: return vvc_dct2_32; default: return vvc_dct2_64; } }
  if( type == 1 ) { switch( n ) { case 4: return vvc_dct8_4; case 8: return vvc_dct8_8; case 16: return vvc_dct8_16; default: return vvc_dct8_32; } }
  switch( n ) { case 4: return vvc_dst7_4; case 8: return vvc_dst7_8; case 16: return vvc_dst7_16; default: return vvc_dst7_32; }
}
static int clip16( int64_t v ) { return (int) std::min<int64_t>( 32767, std::max<int64_t>( -32768, v ) ); }
static int itrAt( int k, int j, int n ) { return ( ( ( k >> 1 ) * n + j ) << 1 ) + ( k & 1 ); }
static uint32_t itrPack( int lo, int hi ) { return ( (uint32_t) lo & 0xffffu ) | ( (uint32_t) hi << 16 ); }
static int dot2( uint32_t a, uint32_t b, int c )
{
  const int64_t s = (int64_t) (int16_t) ( a & 0xffff ) * (int16_t) ( b & 0xffff ) + (int64_t) (int16_t) ( a >> 16 ) * (int16_t) ( b >> 16 ) + c;
  CHECK( s >= INT32_MIN && s <= INT32_MAX, "a sum leaves 32 bits" );
  return (int) s;
}
static int mul24( int a, int b ) { CHECK( a >= -( 1 << 23 ) && a < ( 1 << 23 ) && b >= -( 1 << 23 ) && b < ( 1 << 23 ), "operand of the 24-bit multiply" ); return a * b; }

// One block through the kernel's loops.  dq: the dequantised levels dq[y * bw + x] (what the kernel's dequantisation / LFNST leave); cutH rows and redW columns take part.
static void replayBlock( int MAXN, int NT, int bw, int bh, int trHor, int trVer, int cutH, int redW, int bd, const std::vector<int16_t>& dq, std::vector<int>& out )
{
  const int CUT = MAXN > 32 ? 32 : MAXN;
  const int lw = ilog2i( bw ), lh = ilog2i( bh ), n = bw * bh;
  const bool oneD = bw == 1 || bh == 1;
  const bool fourRows = bh >= 4 && !oneD;
  const int shift1 = 7, shift2 = 20 - bd;
  // heap arrays of exactly the kernel's sizes, garbage in them
  std::vector<uint32_t> dqP( CUT * CUT / 2, 0x7fff8000u ), tmpP( CUT * MAXN / 2, 0x80007fffu ), mvP( CUT * MAXN / 2, 0x7fff7fffu ), mhP( CUT * MAXN / 2, 0x80008000u );
  int16_t* dq16 = reinterpret_cast<int16_t*>( dqP.data() ); int16_t* tmp16 = reinterpret_cast<int16_t*>( tmpP.data() );
  const int16_t* mv16 = reinterpret_cast<const int16_t*>( mvP.data() ); const int16_t* mh16 = reinterpret_cast<const int16_t*>( mhP.data() );
  const int16_t* Mv = nullptr; const int16_t* Mh = nullptr; int cntH = 0;
  if( oneD ) { const int n1 = bw == 1 ? bh : bw; Mh = trMatrix( bw == 1 ? trVer : trHor, n1 ); cntH = redW * n1; cutH = 0; }
  else { Mv = trMatrix( trVer, bh ); Mh = trMatrix( trHor, bw ); cntH = redW * bw; }
  const int ITER_P = CUT * CUT / 2 / NT, ITER_M = CUT * MAXN / 4 / NT, ITER_E = MAXN * MAXN / 4 / NT;
  const int dqW = std::min( bw, CUT ), dqH = std::min( bh, CUT ), ldW = std::min( lw, ilog2i( CUT ) ), dqHp = ( dqH + 1 ) >> 1;
  // levels: a pair of rows of one column per work item
  for( int tid = 0; tid < NT; tid++ ) for( int k = 0; k < ITER_P; k++ )
  {
    const int i = tid + k * NT, yp = i >> ldW, x = i & ( dqW - 1 );
    int o[2];
    for( int e = 0; e < 2; e++ ) { const int y = 2 * yp + e; o[e] = ( y < dqH && y < bh && x < bw ) ? dq[y * bw + x] : 0; }
    if( yp < dqHp ) dqP.at( i ) = itrPack( o[0], o[1] );
  }
  // basis rows: two neighbouring columns of a pair of rows per work item
  const int nV = bh, nH = oneD ? ( bw == 1 ? bh : bw ) : bw, lnV2 = std::max( lh - 1, 0 ), lnH2 = ilog2i( nH ) - 1;
  const int unitsV = ( ( cutH + 1 ) >> 1 ) << lnV2, unitsH = cntH ? ( ( redW + 1 ) >> 1 ) << lnH2 : 0;
  for( int tid = 0; tid < NT; tid++ ) for( int k = 0; k < ITER_M; k++ )
  {
    const int j = tid + k * NT;
    if( j < unitsV )
    {
      const int kp = j >> lnV2, jp = j & ( ( nV >> 1 ) - 1 );
      uint32_t a, b = 0;
      memcpy( &a, Mv + 2 * ( ( ( 2 * kp ) << lnV2 ) + jp ), 4 );
      if( 2 * kp + 1 < cutH ) memcpy( &b, Mv + 2 * ( ( ( 2 * kp + 1 ) << lnV2 ) + jp ), 4 );
      mvP.at( 2 * j ) = ( a & 0xffffu ) | ( b << 16 ); mvP.at( 2 * j + 1 ) = ( a >> 16 ) | ( b & 0xffff0000u );
    }
    if( j < unitsH )
    {
      const int kp = j >> lnH2, jp = j & ( ( nH >> 1 ) - 1 );
      uint32_t a, b = 0;
      memcpy( &a, Mh + 2 * ( ( ( 2 * kp ) << lnH2 ) + jp ), 4 );
      if( 2 * kp + 1 < redW ) memcpy( &b, Mh + 2 * ( ( ( 2 * kp + 1 ) << lnH2 ) + jp ), 4 );
      mhP.at( 2 * j ) = ( a & 0xffffu ) | ( b << 16 ); mhP.at( 2 * j + 1 ) = ( a >> 16 ) | ( b & 0xffff0000u );
    }
  }
  CHECK( (size_t) std::max( unitsV, unitsH ) <= (size_t) ITER_M * NT, "basis rows of %dx%d do not fit the loop", bw, bh );
  // pass 1
  if( !oneD )
  {
    if( bw >= 4 )
    {
      const int grpX = ( redW + 3 ) >> 2, kp1 = ( cutH + 1 ) >> 1;
      for( int tid = 0; tid < NT; tid++ ) for( int i = tid; i < grpX * bh; i += NT )
      {
        const int xg = i >> lh, y = i & ( bh - 1 ), x0 = xg << 2;
        int s[4] = { 0, 0, 0, 0 };
        for( int kp = 0; kp < kp1; kp++ )
        {
          const uint32_t m = mvP.at( kp * bh + y );
          for( int r = 0; r < 4; r++ ) s[r] = dot2( dqP.at( kp * dqW + x0 + r ), m, s[r] );
        }
        int tv[4];
        for( int r = 0; r < 4; r++ ) tv[r] = x0 + r < redW ? clip16( ( s[r] + ( 1 << ( shift1 - 1 ) ) ) >> shift1 ) : 0;
        tmpP.at( ( xg * 2 ) * bh + y ) = itrPack( tv[0], tv[1] ); tmpP.at( ( xg * 2 + 1 ) * bh + y ) = itrPack( tv[2], tv[3] );
      }
    }
    else
      for( int tid = 0; tid < NT; tid++ ) for( int i = tid; i < redW * bh; i += NT )
      {
        const int x = i >> lh, y = i & ( bh - 1 );
        int sum = 0;
        for( int k = 0; k < cutH; k++ ) sum += mul24( dq16[itrAt( k, x, dqW )], mv16[itrAt( k, y, bh )] );
        tmp16[itrAt( x, y, bh )] = (int16_t) clip16( ( sum + ( 1 << ( shift1 - 1 ) ) ) >> shift1 );
      }
  }
  // pass 2
  out.assign( n, 0 );
  if( fourRows )
  {
    const int nItems = ( bh >> 2 ) * bw;
    CHECK( nItems <= ITER_E * NT, "output items of %dx%d do not fit the loop", bw, bh );
    for( int tid = 0; tid < NT; tid++ ) for( int e = 0; e < ITER_E; e++ )
    {
      const int i = tid + e * NT;
      if( i >= nItems ) continue;
      const int yg = i >> lw, x = i & ( bw - 1 ), y0 = yg << 2;
      int s[4] = { 0, 0, 0, 0 };
      for( int kp = 0; kp < ( ( redW + 1 ) >> 1 ); kp++ )
      {
        const uint32_t m = mhP.at( kp * bw + x );
        for( int r = 0; r < 4; r++ ) s[r] = dot2( tmpP.at( kp * bh + y0 + r ), m, s[r] );
      }
      for( int r = 0; r < 4; r++ ) out[( y0 + r ) * bw + x] = clip16( ( s[r] + ( 1 << ( shift2 - 1 ) ) ) >> shift2 );
    }
    return;
  }
  for( int tid = 0; tid < NT; tid++ ) for( int i = tid; i < n; i += NT )
  {
    const int y = i >> lw, x = i & ( bw - 1 );
    int sum = 0;
    if( oneD )
    {
      const int n1 = bw == 1 ? bh : bw;
      for( int k = 0; k < redW; k++ ) sum += mul24( dq16[bw == 1 ? itrAt( k, 0, 1 ) : itrAt( 0, k, dqW )], mh16[itrAt( k, i, n1 )] );
      out[i] = clip16( ( sum + ( 1 << shift2 ) ) >> ( shift2 + 1 ) );
    }
    else
    {
      for( int k = 0; k < redW; k++ ) sum += mul24( tmp16[itrAt( k, y, bh )], mh16[itrAt( k, x, bw )] );
      out[i] = clip16( ( sum + ( 1 << ( shift2 - 1 ) ) ) >> shift2 );
    }
  }
}

// the plain triple loop (fastInvCore_ twice, or once for a 1-D block)
static void plainBlock( int bw, int bh, int trHor, int trVer, int cutH, int redW, int bd, const std::vector<int16_t>& dq, std::vector<int>& out )
{
  const int shift1 = 7, shift2 = 20 - bd;
  out.assign( bw * bh, 0 );
  if( bw == 1 || bh == 1 )
  {
    const int n1 = bw == 1 ? bh : bw; const int16_t* M = trMatrix( bw == 1 ? trVer : trHor, n1 );
    for( int i = 0; i < n1; i++ ) { int64_t s = 0; for( int k = 0; k < redW; k++ ) s += (int64_t) dq[k] * M[k * n1 + i]; out[i] = clip16( ( s + ( 1 << shift2 ) ) >> ( shift2 + 1 ) ); }
    return;
  }
  const int16_t* Mv = trMatrix( trVer, bh ); const int16_t* Mh = trMatrix( trHor, bw );
  std::vector<int> tmp( bw * bh, 0 );
  for( int x = 0; x < redW; x++ ) for( int y = 0; y < bh; y++ ) { int64_t s = 0; for( int k = 0; k < cutH; k++ ) s += (int64_t) dq[k * bw + x] * Mv[k * bh + y]; tmp[x * bh + y] = clip16( ( s + 64 ) >> shift1 ); }
  for( int y = 0; y < bh; y++ ) for( int x = 0; x < bw; x++ ) { int64_t s = 0; for( int k = 0; k < redW; k++ ) s += (int64_t) tmp[k * bh + y] * Mh[k * bw + x]; out[y * bw + x] = clip16( ( s + ( 1 << ( shift2 - 1 ) ) ) >> shift2 ); }
}

static uint32_t rngState = 12345;
static uint32_t rnd() { rngState = rngState * 1664525u + 1013904223u; return rngState >> 8; }

static size_t checkPasses()
{
  static const int sizes[7] = { 1, 2, 4, 8, 16, 32, 64 };
  size_t blocks = 0;
  std::vector<int16_t> dq; std::vector<int> got, want;
  for( int bw : sizes ) for( int bh : sizes )
  {
    if( bw == 1 && bh == 1 ) continue;
    const bool oneD = bw == 1 || bh == 1;
    if( oneD && bw * bh < 16 ) continue;                    // (1-D blocks are the partitions of 4xN / Nx4 ISP CUs of at least 16 samples)
    if( ( bw == 2 || bh == 2 ) && std::max( bw, bh ) > 32 ) continue;      // (2-wide blocks are chroma of 4-wide CUs: at most 2 x 32)
    const int m = std::max( bw, bh ), MAXN = m <= 16 ? 16 : m <= 32 ? 32 : 64, NT = MAXN == 16 ? 64 : MAXN == 32 ? 128 : 256;
    for( int trHor = 0; trHor < 3; trHor++ ) for( int trVer = 0; trVer < 3; trVer++ )
    {
      if( trHor && ( bw < 4 || bw > 32 ) && bw != 1 ) continue;
      if( trVer && ( bh < 4 || bh > 32 ) && bh != 1 ) continue;
      if( bw == 1 && trHor ) continue;
      if( bh == 1 && trVer ) continue;
      const int maxW = bw == 1 ? 1 : ( trHor && bw == 32 ) ? 16 : std::min( bw, 32 ), maxH = bh == 1 ? 1 : ( trVer && bh == 32 ) ? 16 : std::min( bh, 32 );
      for( int cutH = 1; cutH <= maxH; cutH++ ) for( int redW = 1; redW <= maxW; redW++ )
      {
        // every count of one direction with a few of the other: the smallest, odd and even ones in the middle, the two largest
        const bool fewW = redW <= 3 || redW >= maxW - 1 || redW == maxW / 2 || redW == maxW / 2 + 1, fewH = cutH <= 3 || cutH >= maxH - 1 || cutH == maxH / 2 || cutH == maxH / 2 + 1;
        if( !fewW && !fewH ) continue;
        for( int pattern = 0; pattern < 3; pattern++ )
        {
          if( pattern < 2 && !( fewW && fewH ) ) continue;       // (the two constant patterns: with the few counts of both directions; the mixed one: with every count)
          dq.assign( bw * bh, 0 );
          // the levels the kernel's dequantisation leaves: anything in the corner that takes part AND beyond it (rows / columns the passes must ignore)
          for( int y = 0; y < bh; y++ ) for( int x = 0; x < bw; x++ )
            dq[y * bw + x] = (int16_t) ( pattern == 0 ? 32767 : pattern == 1 ? -32768 : ( rnd() & 3 ) == 0 ? ( ( rnd() & 1 ) ? 32767 : -32768 ) : (int) ( rnd() & 0xffff ) - 32768 );
          const int bd = pattern == 1 ? 8 : 10;
          // a 1-D block: its only pass takes `redW` rows of the basis, counted along its only dimension
          const int cH = oneD ? 0 : cutH, rW = oneD ? ( bw == 1 ? cutH : redW ) : redW;
          replayBlock( MAXN, NT, bw, bh, trHor, trVer, cH, rW, bd, dq, got );
          plainBlock( bw, bh, trHor, trVer, cH, rW, bd, dq, want );
          if( got != want ) CHECK( false, "%dx%d transform %d/%d, %d rows and %d columns take part, pattern %d", bw, bh, trHor, trVer, cH, rW, pattern );
          blocks++;
        }
      }
    }
  }
  return blocks;
}

int main( int argc, char** argv )
{
  size_t recs = 0;
  for( int i = 1; i < argc; i++ ) recs += checkRecords( argv[i] );
  const size_t blocks = checkPasses();
  printf( "%zu records, %zu blocks\n", recs, blocks );
  if( failures ) { printf( "%d checks failed\n", failures ); return 1; }
  printf( "all equal\n" );
  return 0;
}
