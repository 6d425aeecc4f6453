// TEST INFRASTRUCTURE (tests/ only): the lane structure of k_hash_rows / k_hash_combine (vvdec_amd/csrc/vvr_kernels.hip) restated for the CPU -
// lanes as loops, __shfl_down as an array read (a lane beyond the wavefront reads itself), LDS as arrays - so that what the plain-loop
// launchers of the stand-in runtime do not exercise is checked without a GPU: the byte tables, the chunks numbered from the end of a row's
// whole chunks, the Horner step per chunk, the six multiply-and-shuffle steps, the tail chunk, the h + 1 pieces of the combine over 256
// threads, the strided checksum lanes, and the powers of x as vvr_output.inc's hash_params computes them.  It restates the kernels, it does
// not compile them: a change to the kernels has to be made here as well.  Compared with the CRC fed bit by bit and the checksum sample by
// sample (compCRC / compChecksum, PicYuvMD5.cpp:99-176).  Prints "all equal" and returns 0, or the planes that differ.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <cstring>
typedef int16_t pel_t;
static uint32_t crcMul( uint32_t a, uint32_t b ) { uint32_t r = 0; for( int bit = 15; bit >= 0; bit-- ) { r <<= 1; if( r & 0x10000 ) r ^= 0x11021; if( ( b >> bit ) & 1 ) r ^= a; } return r; }
static uint32_t crcXPow( uint64_t n ) { uint32_t r = 1, base = 2; while( n ) { if( n & 1 ) r = crcMul( r, base ); base = crcMul( base, base ); n >>= 1; } return r; }
static uint32_t crc_mul( uint32_t a, uint32_t b ) { uint32_t r = 0; for( int bit = 15; bit >= 0; bit-- ) { r <<= 1; r ^= ( ( r >> 16 ) & 1 ) * 0x11021u; r ^= ( ( b >> bit ) & 1 ) * a; } return r; }
struct HashParams { const pel_t* src[3]; int stride[3], w[3], h[3]; int numComp, two, crc; uint32_t xIter, xTree[6], xTail[3]; uint32_t xRowIter[3], xRowTree[3][7]; };
struct uint4 { uint32_t x, y, z, w; };
static uint16_t tbl[14][256];
static uint32_t term( int K, uint32_t byte ) { return K == 0 ? byte : K == 1 ? byte << 8 : (uint32_t) tbl[K - 2][byte]; }
static uint32_t sample( bool TWO, int I, uint32_t v ) { if( TWO ) return term( 15 - 2 * I, v & 0xff ) ^ term( 14 - 2 * I, v >> 8 ); return term( 7 - I, v & 0xff ); }
static uint32_t chunk( bool TWO, uint4 q ) { return sample( TWO, 0, q.x & 0xffff ) ^ sample( TWO, 1, q.x >> 16 ) ^ sample( TWO, 2, q.y & 0xffff ) ^ sample( TWO, 3, q.y >> 16 ) ^ sample( TWO, 4, q.z & 0xffff ) ^ sample( TWO, 5, q.z >> 16 ) ^ sample( TWO, 6, q.w & 0xffff ) ^ sample( TWO, 7, q.w >> 16 ); }
static void shfl_tree( uint32_t acc[64], const uint32_t* x )
{
  for( int s = 0; s < 6; s++ ) { uint32_t nxt[64]; for( int l = 0; l < 64; l++ ) nxt[l] = acc[l + ( 1 << s ) < 64 ? l + ( 1 << s ) : l]; for( int l = 0; l < 64; l++ ) acc[l] = crc_mul( acc[l], x[s] ) ^ nxt[l]; }
}
static void rowsKernel( const HashParams& p, bool TWO, uint32_t* rows )
{
  for( int t = 0; t < 256; t++ ) { uint32_t a = t << 8; for( int k = 0; k < ( TWO ? 14 : 6 ); k++ ) { for( int i = 0; i < 8; i++ ) { a <<= 1; a ^= ( ( a >> 16 ) & 1 ) * 0x11021u; } tbl[k][t] = (uint16_t) a; } }
  int rowsTotal = 0; for( int c = 0; c < p.numComp; c++ ) rowsTotal += p.h[c];
  for( int g = 0; g < rowsTotal; g++ )
  {
    int c = 0, y = g; if( y >= p.h[0] ) { y -= p.h[0]; c = 1; if( y >= p.h[1] ) { y -= p.h[1]; c = 2; } }
    const int w = p.w[c]; const pel_t* row = p.src[c] + (size_t) y * p.stride[c];
    const int nFull = w >> 3, rem = w & 7;
    uint32_t acc[64] = { 0 };
    const int nIter = ( nFull + 63 ) >> 6, pad = nIter * 64 - nFull;
    for( int it = 0; it < nIter; it++ ) for( int lane = 0; lane < 64; lane++ )
    {
      const int ci = it * 64 + lane - pad; uint32_t v = 0;
      if( ci >= 0 ) { uint4 q; memcpy( &q, row + 8 * ci, 16 ); v = chunk( TWO, q ); }
      acc[lane] = crc_mul( acc[lane], p.xIter ) ^ v;
    }
    shfl_tree( acc, p.xTree );
    if( rem )
    {
      uint32_t t[8]; for( int i = 0; i < 8; i++ ) t[i] = i >= 8 - rem ? (uint32_t) (uint16_t) row[w - 8 + i] : 0u;
      uint4 q; q.x = t[0] | t[1] << 16; q.y = t[2] | t[3] << 16; q.z = t[4] | t[5] << 16; q.w = t[6] | t[7] << 16;
      acc[0] = crc_mul( acc[0], p.xTail[c] ) ^ chunk( TWO, q );
    }
    rows[g] = acc[0];
  }
}
static void combineKernel( const HashParams& p, const uint32_t* rowsAll, uint32_t* out )
{
  for( int c = 0; c < p.numComp; c++ )
  {
    const int h = p.h[c]; const uint32_t* rows = rowsAll + ( c == 0 ? 0 : c == 1 ? p.h[0] : p.h[0] + p.h[1] );
    uint32_t acc[256] = { 0 }, part[4];
    const int n = h + 1, nIter = ( n + 255 ) >> 8, pad = nIter * 256 - n;
    for( int it = 0; it < nIter; it++ ) for( int t = 0; t < 256; t++ ) { const int i = it * 256 + t - pad; acc[t] = crc_mul( acc[t], p.xRowIter[c] ) ^ ( i < 0 ? 0u : i == 0 ? 0xffffu : rows[i - 1] & 0xffffu ); }
    for( int wv = 0; wv < 4; wv++ ) { shfl_tree( acc + 64 * wv, p.xRowTree[c] ); part[wv] = acc[64 * wv]; }
    uint32_t a = part[0]; for( int k = 1; k < 4; k++ ) a = crc_mul( a, p.xRowTree[c][6] ) ^ part[k];
    out[c] = crc_mul( a, 0x1021u );
  }
}
static uint32_t sumSample( bool TWO, uint32_t v, int x, int y ) { const uint32_t mask = ( ( x & 0xff ) ^ ( y & 0xff ) ^ ( x >> 8 ) ^ ( y >> 8 ) ) & 0xff; return ( ( v & 0xff ) ^ mask ) + ( TWO ? ( v >> 8 ) ^ mask : 0u ); }
static void rowsKernelSum( const HashParams& p, bool TWO, uint32_t* rows )
{
  int rowsTotal = 0; for( int c = 0; c < p.numComp; c++ ) rowsTotal += p.h[c];
  for( int g = 0; g < rowsTotal; g++ )
  {
    int c = 0, y = g; if( y >= p.h[0] ) { y -= p.h[0]; c = 1; if( y >= p.h[1] ) { y -= p.h[1]; c = 2; } }
    const int w = p.w[c]; const pel_t* row = p.src[c] + (size_t) y * p.stride[c];
    const int nFull = w >> 3, rem = w & 7;
    uint32_t acc[64] = { 0 };
    for( int lane = 0; lane < 64; lane++ )
    {
      for( int ci = lane; ci < nFull; ci += 64 ) for( int i = 0; i < 8; i++ ) acc[lane] += sumSample( TWO, (uint16_t) row[8 * ci + i], 8 * ci + i, y );
      if( lane < rem ) acc[lane] += sumSample( TWO, (uint16_t) row[8 * nFull + lane], 8 * nFull + lane, y );
    }
    for( int o = 32; o; o >>= 1 ) for( int l = 0; l < 64; l++ ) acc[l] += acc[l + o < 64 ? l + o : l];
    rows[g] = acc[0];
  }
}
static void combineKernelSum( const HashParams& p, const uint32_t* rowsAll, uint32_t* out )
{
  for( int c = 0; c < p.numComp; c++ )
  {
    const uint32_t* rows = rowsAll + ( c == 0 ? 0 : c == 1 ? p.h[0] : p.h[0] + p.h[1] );
    uint32_t acc[256] = { 0 }, part[4];
    for( int t = 0; t < 256; t++ ) for( int r = t; r < p.h[c]; r += 256 ) acc[t] += rows[r];
    for( int wv = 0; wv < 4; wv++ ) { uint32_t* a = acc + 64 * wv; for( int o = 32; o; o >>= 1 ) for( int l = 0; l < 64; l++ ) a[l] += a[l + o < 64 ? l + o : l]; part[wv] = a[0]; }
    out[c] = part[0] + part[1] + part[2] + part[3];
  }
}
static uint32_t refSum( const pel_t* pl, int stride, int w, int h, bool two )
{
  uint32_t s = 0;
  for( int y = 0; y < h; y++ ) for( int x = 0; x < w; x++ ) s += sumSample( two, (uint16_t) pl[(size_t) y * stride + x], x, y );
  return s;
}
static uint32_t refCrc( const pel_t* pl, int stride, int w, int h, bool two )
{
  uint32_t crc = 0xffff;
  auto feed = [&]( uint32_t byte ) { for( int bit = 7; bit >= 0; bit-- ) { const uint32_t msb = ( crc >> 15 ) & 1; crc = ( ( ( crc << 1 ) + ( ( byte >> bit ) & 1 ) ) & 0xffff ) ^ ( msb * 0x1021 ); } };
  for( int y = 0; y < h; y++ ) for( int x = 0; x < w; x++ ) { const uint32_t v = (uint16_t) pl[(size_t) y * stride + x]; feed( v & 0xff ); if( two ) feed( v >> 8 ); }
  for( int i = 0; i < 2; i++ ) feed( 0 );
  return crc;
}
int main()
{
  const int shapes[][4] = { { 200, 72, 3, 10 }, { 72, 136, 3, 8 }, { 136, 8, 1, 10 }, { 7680, 16, 3, 10 }, { 8, 2, 3, 10 }, { 6, 2, 1, 8 }, { 1032, 300, 3, 10 }, { 520, 1100, 3, 8 } };
  int bad = 0;
  for( auto& sh : shapes )
  {
    const int W = sh[0], H = sh[1], nc = sh[2], bd = sh[3]; const bool two = bd > 8;
    HashParams p; memset( &p, 0, sizeof( p ) );
    std::vector<std::vector<pel_t>> planes( nc );
    for( int k = 0; k < nc; k++ )
    {
      p.w[k] = k ? W / 2 : W; p.h[k] = k ? H / 2 : H; p.stride[k] = ( p.w[k] + 63 ) / 64 * 64;
      planes[k].resize( (size_t) p.stride[k] * p.h[k] ); for( auto& v : planes[k] ) v = (pel_t) ( rand() & ( ( 1 << bd ) - 1 ) );
      p.src[k] = planes[k].data();
    }
    p.numComp = nc; p.two = two; p.crc = 1;
    const uint64_t bits = two ? 16 : 8, ch = 8 * bits;
    p.xIter = crcXPow( 64 * ch ); for( int s = 0; s < 6; s++ ) p.xTree[s] = crcXPow( ch << s );
    for( int k = 0; k < nc; k++ ) { const uint64_t row = (uint64_t) p.w[k] * bits; p.xTail[k] = crcXPow( ( p.w[k] & 7 ) * bits ); p.xRowIter[k] = crcXPow( row * 256 ); for( int s = 0; s < 7; s++ ) p.xRowTree[k][s] = crcXPow( row << s ); }
    std::vector<uint32_t> rows( 3 * H ); uint32_t out[3];
    rowsKernel( p, two, rows.data() ); combineKernel( p, rows.data(), out );
    for( int k = 0; k < nc; k++ ) { const uint32_t want = refCrc( p.src[k], p.stride[k], p.w[k], p.h[k], two ); if( want != out[k] ) { bad++; printf( "%dx%d comp %d: CRC %04x want %04x\n", W, H, k, out[k], want ); } }
    rowsKernelSum( p, two, rows.data() ); combineKernelSum( p, rows.data(), out );
    for( int k = 0; k < nc; k++ ) { const uint32_t want = refSum( p.src[k], p.stride[k], p.w[k], p.h[k], two ); if( want != out[k] ) { bad++; printf( "%dx%d comp %d: checksum %08x want %08x\n", W, H, k, out[k], want ); } }
  }
  printf( bad ? "FAILED\n" : "all equal\n" );
  return bad;
}
