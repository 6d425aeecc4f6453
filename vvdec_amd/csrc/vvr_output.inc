// vvdec_amd/csrc/vvr_output.inc — output stage at the boundary (included by vvr_api.cpp): what the reference does to a finished picture on its way
// to the application (VVDecImpl::xAddPicture / copyComp, vvdecimpl.cpp:818-1060: conformance-window crop, 8-bit narrowing) and the decoded
// picture hash it checks against the SEI (PicYuvMD5.cpp:99-260).  Crop, narrowing, CRC and checksum run on the device, so a picture only
// crosses PCIe in the form the application asked for (or not at all when only its digest is wanted); MD5 is a serial chain over the bytes of a
// plane and stays on the host.

namespace {
struct Md5     // RFC 1321
{
  uint32_t a = 0x67452301u, b = 0xefcdab89u, c = 0x98badcfeu, d = 0x10325476u; uint64_t len = 0; uint8_t buf[64]; size_t fill = 0;
  static uint32_t rol( uint32_t v, int s ) { return ( v << s ) | ( v >> ( 32 - s ) ); }
  void block( const uint8_t* p )
  {
    static const uint32_t K[64] = {
      0xd76aa478,0xe8c7b756,0x242070db,0xc1bdceee,0xf57c0faf,0x4787c62a,0xa8304613,0xfd469501,0x698098d8,0x8b44f7af,0xffff5bb1,0x895cd7be,0x6b901122,0xfd987193,0xa679438e,0x49b40821,
      0xf61e2562,0xc040b340,0x265e5a51,0xe9b6c7aa,0xd62f105d,0x02441453,0xd8a1e681,0xe7d3fbc8,0x21e1cde6,0xc33707d6,0xf4d50d87,0x455a14ed,0xa9e3e905,0xfcefa3f8,0x676f02d9,0x8d2a4c8a,
      0xfffa3942,0x8771f681,0x6d9d6122,0xfde5380c,0xa4beea44,0x4bdecfa9,0xf6bb4b60,0xbebfbc70,0x289b7ec6,0xeaa127fa,0xd4ef3085,0x04881d05,0xd9d4d039,0xe6db99e5,0x1fa27cf8,0xc4ac5665,
      0xf4292244,0x432aff97,0xab9423a7,0xfc93a039,0x655b59c3,0x8f0ccc92,0xffeff47d,0x85845dd1,0x6fa87e4f,0xfe2ce6e0,0xa3014314,0x4e0811a1,0xf7537e82,0xbd3af235,0x2ad7d2bb,0xeb86d391 };
    static const int S[64] = { 7,12,17,22,7,12,17,22,7,12,17,22,7,12,17,22, 5,9,14,20,5,9,14,20,5,9,14,20,5,9,14,20, 4,11,16,23,4,11,16,23,4,11,16,23,4,11,16,23, 6,10,15,21,6,10,15,21,6,10,15,21,6,10,15,21 };
    uint32_t m[16]; for( int i = 0; i < 16; i++ ) m[i] = (uint32_t) p[4 * i] | ( (uint32_t) p[4 * i + 1] << 8 ) | ( (uint32_t) p[4 * i + 2] << 16 ) | ( (uint32_t) p[4 * i + 3] << 24 );
    uint32_t A = a, B = b, C = c, D = d;
    for( int i = 0; i < 64; i++ )
    {
      uint32_t f; int g;
      if( i < 16 ) { f = ( B & C ) | ( ~B & D ); g = i; } else if( i < 32 ) { f = ( D & B ) | ( ~D & C ); g = ( 5 * i + 1 ) & 15; }
      else if( i < 48 ) { f = B ^ C ^ D; g = ( 3 * i + 5 ) & 15; } else { f = C ^ ( B | ~D ); g = ( 7 * i ) & 15; }
      const uint32_t t = D; D = C; C = B; B = B + rol( A + f + K[i] + m[g], S[i] ); A = t;
    }
    a += A; b += B; c += C; d += D;
  }
  void update( const uint8_t* p, size_t n )
  {
    len += n;
    while( n ) { const size_t k = std::min( n, 64 - fill ); memcpy( buf + fill, p, k ); fill += k; p += k; n -= k; if( fill == 64 ) { block( buf ); fill = 0; } }
  }
  void finish( uint8_t out[16] )
  {
    const uint64_t bits = len * 8; const uint8_t one = 0x80, zero = 0;
    update( &one, 1 ); while( fill != 56 ) update( &zero, 1 );
    uint8_t l[8]; for( int i = 0; i < 8; i++ ) l[i] = (uint8_t) ( bits >> ( 8 * i ) );
    update( l, 8 );
    const uint32_t v[4] = { a, b, c, d }; for( int i = 0; i < 16; i++ ) out[i] = (uint8_t) ( v[i >> 2] >> ( 8 * ( i & 3 ) ) );
  }
};

// arithmetic of the CRC's polynomial ring GF(2)[x] / (x^16 + x^12 + x^5 + 1): the CRC register after feeding a message M of N bits from the
// initial value I is ( I * x^N + M ) mod P, so the CRCs of pieces (computed on the device from 0) combine with a multiplication by a power of x
uint32_t crcMul( uint32_t a, uint32_t b )
{
  uint32_t r = 0;
  for( int bit = 15; bit >= 0; bit-- ) { r <<= 1; if( r & 0x10000 ) r ^= 0x11021; if( ( b >> bit ) & 1 ) r ^= a; }
  return r;
}
uint32_t crcXPow( uint64_t n ) { uint32_t r = 1, base = 2; while( n ) { if( n & 1 ) r = crcMul( r, base ); base = crcMul( base, base ); n >>= 1; } return r; }
// what k_hash_rows / k_hash_combine get of a picture: its planes and, for the CRC, the powers of x they multiply by (vvr_device.h).  A row of
// 7680 10-bit samples has 122 880 bits: the exponents are 64-bit here and never formed on the device
HashParams hash_params( const DevPlanes& d, int nc, bool two, bool crc )
{
  HashParams p; memset( &p, 0, sizeof( p ) );
  const uint64_t bits = two ? 16 : 8, chunk = 8 * bits;
  for( int k = 0; k < nc; k++ ) { p.src[k] = d.p[k]; p.stride[k] = d.stride[k]; p.w[k] = d.w[k]; p.h[k] = d.h[k]; }
  p.numComp = nc; p.two = two; p.crc = crc;
  if( !crc ) return p;
  p.xIter = crcXPow( 64 * chunk );
  for( int s = 0; s < 6; s++ ) p.xTree[s] = crcXPow( chunk << s );
  for( int k = 0; k < nc; k++ )
  {
    const uint64_t row = (uint64_t) d.w[k] * bits;
    p.xTail[k] = crcXPow( ( d.w[k] & 7 ) * bits ); p.xRowIter[k] = crcXPow( row * 256 );
    for( int s = 0; s < 7; s++ ) p.xRowTree[k][s] = crcXPow( row << s );
  }
  return p;
}

int ensureOutputScratch( vvr_context* c, size_t devBytes, size_t hostBytes )
{
  if( devBytes > c->outDevCap ) { if( c->outDev ) hipFree( c->outDev ); c->outDev = nullptr; c->outDevCap = 0; HIPCHK( c, hipMalloc( &c->outDev, devBytes ) ); c->outDevCap = devBytes; }
  if( hostBytes > c->outHostCap ) { if( c->outHost ) hipHostFree( c->outHost ); c->outHost = nullptr; c->outHostCap = 0; HIPCHK( c, hipHostMalloc( &c->outHost, hostBytes, hipHostMallocDefault ) ); c->outHostCap = hostBytes; }
  return VVR_OK;
}

// the kernels of the output stage between two events of their own when statistics are on: outTimeBegin before the launch, t.b recorded behind it,
// outTimeEnd once both are complete
void outTimeBegin( vvr_context* c, hipStream_t s, bool& timed, PendingTiming& t, int kernel, double bytes )
{
  if( !c->statsOn || hipEventCreate( &t.a ) != hipSuccess ) return;
  if( hipEventCreate( &t.b ) != hipSuccess ) { hipEventDestroy( t.a ); return; }
  timed = true; t.kernel = kernel; t.bytes = bytes; hipEventRecord( t.a, s );
}
void outTimeEnd( vvr_context* c, bool& timed, PendingTiming& t, int launches = 1 )
{
  if( !timed ) return;
  float ms = 0; hipEventElapsedTime( &ms, t.a, t.b );
  Stat& st = c->stats[t.kernel];
  st.launches += launches; st.ms += ms; st.bytes += t.bytes;
  hipEventDestroy( t.a ); hipEventDestroy( t.b ); timed = false;
}

// the positions of sampleRateConvCore (Buffer.cpp:249-255) for one direction: scale factor from the plane's own sizes ((src << 14) + dst / 2) / dst
// (vvdecimpl.cpp:1633), refPos = ( ( i << cs ) * scale + add ) >> shift, integer part and phase from refPos.  With sides <= 8192 and src / dst in
// [1/8, 8]: scale <= 8 << 14, ( 8191 << 1 ) * scale + add <= 2 147 279 360 < 2^31 - 1
void rescale_axis( int src, int dst, int cs, int collocated, int fracShift, int& scale, int& add, int& shift )
{
  scale = ( ( src << 14 ) + ( dst >> 1 ) ) / dst;
  shift = 14 - fracShift + cs;
  add = ( 1 << ( shift - 1 ) ) + ( ( ( 1 - collocated ) * 8 * ( scale - ( 1 << 14 ) ) + ( 1 << ( 2 + cs ) ) ) >> ( 3 + cs ) );
}

// the taps of output sample i of an axis of n source and m output samples under a filter of vvr_set_output_resampling, the definition of vvr.h
// term by term in 64-bit integers (n, m, phi, i checked by the caller: 1 <= n, m <= 8192, n <= 64 m, m <= 8 n).  Returns the count, 0 when
// the definition gives no tap list (it does not inside the accepted range)
int64_t floorDiv( int64_t a, int64_t b ) { const int64_t q = a / b; return ( a % b != 0 && ( ( a < 0 ) != ( b < 0 ) ) ) ? q - 1 : q; }      // b > 0 throughout
int resample_taps_of( int filter, int n, int m, int phi, int i, int& first, int16_t* w )
{
  int a = n, b = m; while( b ) { const int t = a % b; a = b; b = t; }
  const int64_t n1 = n / a, m1 = m / a, S = 4 * std::max( n1, m1 ), Q = ( 4 * (int64_t) i + phi ) * n1;
  int64_t num[VVR_RESAMPLE_MAX_TAPS], kLo, kHi;
  if( filter == VVR_RESAMPLE_AREA )
  {
    // the boxes tile the line: box k = [ 4 k m' + ( phi - 2 ) m', 4 ( k + 1 ) m' + ( phi - 2 ) m' ); the two outermost take what lies beyond them
    const int64_t lo = Q - 2 * n1, hi = Q + 2 * n1, base = ( phi - 2 ) * m1;
    kLo = std::min<int64_t>( std::max<int64_t>( floorDiv( lo - base, 4 * m1 ), 0 ), n - 1 ); kHi = std::max<int64_t>( std::min<int64_t>( floorDiv( hi - 1 - base, 4 * m1 ), n - 1 ), 0 );
    if( kHi - kLo + 1 > VVR_RESAMPLE_MAX_TAPS ) return 0;
    for( int64_t k = kLo; k <= kHi; k++ )
    {
      const int64_t from = k == 0 ? lo : std::max( lo, 4 * k * m1 + base ), to = k == n - 1 ? hi : std::min( hi, 4 * ( k + 1 ) * m1 + base );
      num[k - kLo] = to - from;
    }
  }
  else
  {
    const int64_t R = filter == VVR_RESAMPLE_CUBIC ? 2 * S : S;      // N < R: Q - R < P_k < Q + R
    kLo = std::max<int64_t>( -floorDiv( -( Q - R + 1 - phi * m1 ), 4 * m1 ), 0 ); kHi = std::min<int64_t>( floorDiv( Q + R - 1 - phi * m1, 4 * m1 ), n - 1 );
    if( kHi < kLo || kHi - kLo + 1 > VVR_RESAMPLE_MAX_TAPS ) return 0;
    for( int64_t k = kLo; k <= kHi; k++ )
    {
      const int64_t P = ( 4 * k + phi ) * m1, N = P > Q ? P - Q : Q - P;
      num[k - kLo] = filter == VVR_RESAMPLE_TRIANGLE ? S - N : N < S ? 3 * N * N * N - 5 * N * N * S + 2 * S * S * S : -N * N * N + 5 * N * N * S - 8 * N * S * S + 4 * S * S * S;
    }
  }
  const int count = (int) ( kHi - kLo + 1 );
  int64_t T = 0;
  for( int k = 0; k < count; k++ ) T += num[k];
  if( T <= 0 ) return 0;
  int sum = 0, best = 0;
  for( int k = 0; k < count; k++ ) { w[k] = (int16_t) floorDiv( 2 * num[k] * 16384 + T, 2 * T ); sum += w[k]; if( w[k] > w[best] ) best = k; }
  w[best] = (int16_t) ( w[best] + 16384 - sum );
  first = (int) kLo;
  return count;
}
bool resample_axis_ok( int n, int m ) { return n >= 1 && m >= 1 && n <= 8192 && m <= 8192 && n <= 64 * m && m <= 8 * n; }

// the film grain's random generator (prng, FilmGrainImpl.h) and the words of a frame's blocks: FilmGrain::prepareBlockSeeds( w, h ) gives band
// by (16 luma rows) the seed s[by], s[0] the chain's state and s[by + 1] = s[by] after nbx steps; add_grain_line gives block bx of the band s[by]
// after bx steps.  words: nby x nbx.  Returns the chain's state after the frame, the seed of its last band (FilmGrain.cpp:794-820).
uint32_t grain_prng( uint32_t x ) { return ( ( ( x << 30 ) ^ ( x << 2 ) ) & 0x80000000u ) | ( x >> 1 ); }
uint32_t grain_words( uint32_t state, int nbx, int nby, uint32_t* words )
{
  uint32_t seed = state;
  for( int by = 0; by < nby; by++ )
  {
    if( by ) seed = grain_prng( words[(size_t) by * nbx - 1] );
    uint32_t r = seed;
    for( int bx = 0; bx < nbx; bx++ ) { words[(size_t) by * nbx + bx] = r; r = grain_prng( r ); }
  }
  return seed;
}

// the colour description of the RGB formats (vvr.h): Kr, Kb of an H.273 matrix_coefficients code point the queue accepts, and the five Q14
// coefficients cy, rv, gu, gv, bu of a conversion from bd to od bits, q( v ) = floor( v * 16384 + 0.5 ) in double
bool rgb_matrix( int matrix, double& kr, double& kb )
{
  switch( matrix )
  {
  case 1:         kr = 0.2126; kb = 0.0722; return true;      // BT.709
  case 5: case 6: kr = 0.299;  kb = 0.114;  return true;      // BT.601 (625 and 525 lines)
  case 9:         kr = 0.2627; kb = 0.0593; return true;      // BT.2020 non-constant luminance
  }
  return false;
}
void rgb_coefficients( int matrix, int fullRange, int bd, int od, OutputRgbParams& p )
{
  double kr = 0, kb = 0; rgb_matrix( matrix, kr, kb );
  const double kg = 1 - kr - kb, m = ( 1 << od ) - 1, s = 1 << ( bd - 8 );
  const double ys = fullRange ? m / ( ( 1 << bd ) - 1 ) : m / ( 219 * s ), cs = fullRange ? ys : m / ( 224 * s );
  auto q = []( double v ) { return (int) std::floor( v * 16384 + 0.5 ); };
  p.cy = q( ys ); p.rv = q( 2 * ( 1 - kr ) * cs ); p.gu = -q( 2 * kb * ( 1 - kb ) / kg * cs ); p.gv = -q( 2 * kr * ( 1 - kr ) / kg * cs ); p.bu = q( 2 * ( 1 - kb ) * cs );
  p.maxVal = ( 1 << bd ) - 1; p.maxOut = ( 1 << od ) - 1; p.yoff = fullRange ? 0 : 16 << ( bd - 8 ); p.coff = 1 << ( bd - 1 );
  p.inv = 1.0f / (float) ( ( 1 << bd ) - 1 );
}
}   // namespace

#if !defined(__HIPCC__)
// Host builds of this file (the CPU test harness compiles the host code against a stand-in runtime): the launcher as a plain loop restating
// sampleRateConvCore (Buffer.cpp:235-318), so that the host half of vvr_read_output_scaled is checked without a GPU.  The product is always compiled
// by hipcc and takes k_rescale (vvr_kernels.hip).
namespace rescale_host_tbl {
#include "../../tables/vvc_tables.inc"
}
static void rescale_region( const RescaleParams& p, void* dst );
// (the regions of a batch, vvr_output_submit_batch: the loop that is blockIdx.z on the device)
void launch_rescale( hipStream_t, const RescaleParams& p, void* dst, const PlaneRegions& rg )
{
  for( int z = 0; z < rg.count; z++ )
  {
    RescaleParams q = p;
    if( rg.srcOff ) q.src += rg.srcOff[3 * z + rg.comp];
    rescale_region( q, (uint8_t*) dst + (size_t) z * rg.dstStep );
  }
}
static void rescale_region( const RescaleParams& p, void* dst )
{
  const int taps = p.luma ? 8 : 4, fracShift = p.luma ? 4 : 5, fracMask = ( 1 << fracShift ) - 1;
  auto coef = [&]( int frac, int k ) { return (int) ( p.luma ? rescale_host_tbl::vvc_luma_filter[frac][k] : rescale_host_tbl::vvc_chroma_filter[frac][k] ); };
  std::vector<int> tmp( (size_t) p.h * p.outW );
  for( int i = 0; i < p.outW; i++ )
  {
    const int refPos = ( i * p.stepX + p.addX ) >> p.shiftX, integer = refPos >> fracShift, frac = refPos & fracMask;
    for( int j = 0; j < p.h; j++ )
    {
      int sum = 0;
      for( int k = 0; k < taps; k++ ) sum += coef( frac, k ) * p.src[(size_t) j * p.stride + std::min( std::max( 0, integer + k - taps / 2 + 1 ), p.w - 1 )];
      tmp[(size_t) j * p.outW + i] = sum;
    }
  }
  for( int j = 0; j < p.outH; j++ )
  {
    const int refPos = ( j * p.stepY + p.addY ) >> p.shiftY, integer = refPos >> fracShift, frac = refPos & fracMask;
    for( int i = 0; i < p.outW; i++ )
    {
      int sum = 0;
      for( int k = 0; k < taps; k++ ) sum += coef( frac, k ) * tmp[(size_t) std::min( std::max( 0, integer + k - taps / 2 + 1 ), p.h - 1 ) * p.outW + i];
      const int v = std::min( std::max( 0, ( sum + 2048 ) >> 12 ), p.maxVal );
      if( p.bytesPerSample == 2 ) ( (uint16_t*) dst )[(size_t) j * p.outW + i] = (uint16_t) v; else ( (uint8_t*) dst )[(size_t) j * p.outW + i] = (uint8_t) v;
    }
  }
}

// ... and launch_output_resample (k_output_resample): the two passes of vvr_set_output_resampling (vvr.h) sample by sample over the tap tables
// as the device takes them
static void resample_region( const ResampleParams& p, void* dst );
void launch_output_resample( hipStream_t, const ResampleParams& p, void* dst, void*, const PlaneRegions& rg )
{
  for( int z = 0; z < rg.count; z++ )
  {
    ResampleParams q = p;
    if( rg.srcOff ) q.src += rg.srcOff[3 * z + rg.comp];
    resample_region( q, (uint8_t*) dst + (size_t) z * rg.dstStep );
  }
}
static void resample_region( const ResampleParams& p, void* dst )
{
  const int16_t* wx = (const int16_t*) ( p.tabX + p.outW ); const int16_t* wy = (const int16_t*) ( p.tabY + p.outH );
  std::vector<int> H( (size_t) p.h * p.outW );
  for( int r = 0; r < p.h; r++ )
    for( int i = 0; i < p.outW; i++ )
    {
      const int first = p.tabX[i] & 0xffff, count = p.tabX[i] >> 16;
      int sum = 0;
      for( int t = 0; t < count; t++ ) sum += wx[(size_t) t * p.outW + i] * p.src[(size_t) r * p.stride + first + t];
      H[(size_t) r * p.outW + i] = ( sum + 512 ) >> 10;
    }
  for( int j = 0; j < p.outH; j++ )
    for( int i = 0; i < p.outW; i++ )
    {
      const int first = p.tabY[j] & 0xffff, count = p.tabY[j] >> 16;
      int sum = 0;
      for( int t = 0; t < count; t++ ) sum += wy[(size_t) t * p.outH + j] * H[(size_t) ( first + t ) * p.outW + i];
      const int v = std::min( std::max( 0, ( sum + 131072 ) >> 18 ), p.maxVal );
      if( p.bytesPerSample == 2 ) ( (uint16_t*) dst )[(size_t) j * p.outW + i] = (uint16_t) v; else ( (uint8_t*) dst )[(size_t) j * p.outW + i] = (uint8_t) v;
    }
}

// ... and launch_film_grain as a plain loop restating FilmGrainImpl::add_grain_block (FilmGrainImpl.cpp:126-324) row by row: the pre-deblock grain
// of every block of the row (make_grain_pattern), the horizontal deblocking across each block edge, scale, add and clip (scale_and_output)
void launch_film_grain( hipStream_t, const FilmGrainParams& p, void* dst )
{
  const vvr_film_grain_bank& b = *p.bank;
  for( int c = 0; c < p.numComp; c++ )
  {
    const int sub = c ? 2 : 1, bw = 16 / sub, w = p.w[c], n = p.nbx * bw;
    std::vector<int> I( n ), g( n ), d( n );
    for( int r = 0; r < p.h[c]; r++ )
    {
      const pel_t* row = p.src[c] + (size_t) r * p.stride[c];
      for( int x = 0; x < n; x++ ) I[x] = row[std::min( x, w - 1 )];
      std::fill( d.begin(), d.end(), 0 );
      if( b.comp_present[c] )
      {
        const int y = r * sub, j = y & 15;
        const int oc1 = y > 15 && j == 0 ? ( sub > 1 ? 20 : 12 ) : ( y > 15 && j == 1 ? 24 : 0 ), oc2 = y > 15 && j == 0 ? ( sub > 1 ? 20 : 24 ) : 12;
        auto offset = [&]( uint32_t v, int& s, int& ox, int& oy )      // get_offset_y / _u / _v, 4:2:0 chroma
        {
          const uint32_t sx = c == 0 ? 31 : ( c == 1 ? 2 : 15 );
          const uint32_t bx = c == 0 ? v & 0x3ff : ( c == 1 ? ( v >> 10 ) & 0x3ff : ( v >> 20 ) & 0x3ff );
          const uint32_t by = c == 0 ? ( v >> 14 ) & 0x3ff : ( c == 1 ? ( ( v >> 24 ) & 0xff ) | ( ( v << 8 ) & 0x300 ) : ( v >> 4 ) & 0x3ff );
          s = ( v >> sx ) & 1 ? -1 : 1; ox = (int) ( ( bx * 13 ) >> 10 ) * ( 4 / sub ); oy = (int) ( ( by * 12 ) >> 10 ) * ( 4 / sub );
        };
        for( int bx = 0; bx < p.nbx; bx++ )
        {
          int s, ox, oy, sUp = 1, oxUp = 0, oyUp = 0;
          offset( p.words[(size_t) ( y / 16 ) * p.nbx + bx], s, ox, oy ); oy += j / sub;
          if( oc1 ) { offset( p.words[(size_t) ( y / 16 - 1 ) * p.nbx + bx], sUp, oxUp, oyUp ); oyUp += ( 16 + j ) / sub; }
          for( int i = 0; i < bw; i++ )
          {
            const int pi = b.pattern_lut[c][( I[bx * bw + i] >> ( p.bs ) ) & 0xff] >> 4;
            int P = b.pattern[c ? 1 : 0][pi][oy][ox + i] * s;
            if( oc1 ) P = ( P * oc1 + b.pattern[c ? 1 : 0][pi][oyUp][oxUp + i] * oc2 * sUp + 16 ) >> 5;
            g[bx * bw + i] = P;
          }
        }
        d = g;
        for( int e = bw; e < n; e += bw ) { d[e - 1] = ( g[e - 2] + 3 * g[e - 1] + g[e] + 2 ) >> 2; d[e] = ( g[e - 1] + 3 * g[e] + g[e + 1] + 2 ) >> 2; }
      }
      for( int x = 0; x < w; x++ )
      {
        const int v = b.comp_present[c] ? std::min( std::max( 0, I[x] + ( ( b.scale_lut[c][( I[x] >> p.bs ) & 0xff] * d[x] + ( 1 << ( p.scaleShift - 1 ) ) ) >> p.scaleShift ) ), 255 << p.bs ) : I[x];
        uint8_t* out = (uint8_t*) dst + p.dstOff[c] + ( (size_t) r * w + x ) * p.bytesPerSample;
        if( p.bytesPerSample == 2 ) *(uint16_t*) out = (uint16_t) v; else *out = (uint8_t) v;
      }
    }
  }
}

// ... and launch_output_frame: the planes' windows row by row in the five formats (k_output_frame); plane 1 of the semi-planar ones takes its
// samples from the two chroma windows in turn
void launch_output_frame( hipStream_t, OutputFrameParams p, void* dst )
{
  const bool semi = p.format == VVR_OUT_NV12 || p.format == VVR_OUT_P010;
  for( int c = 0; c < 3; c++ )
    for( int r = 0; r < ( p.w[c] ? p.h[c] : 0 ); r++ )
    {
      uint8_t* out = p.direct[c] ? p.direct[c] : (uint8_t*) dst + p.dstOff[c];
      auto sample = [&]( int x ) { const int k = semi && c == 1 ? 1 + ( x & 1 ) : c, col = semi && c == 1 ? x >> 1 : x; return (uint16_t) p.src[k][(size_t) r * p.stride[k] + col]; };
      for( int x = 0; x < p.w[c]; x++ )
      {
        const size_t i = (size_t) r * p.w[c] + x;
        if( p.format == VVR_OUT_PLANAR16 ) ( (uint16_t*) out )[i] = sample( x );
        else if( p.format == VVR_OUT_P010 ) ( (uint16_t*) out )[i] = (uint16_t) ( sample( x ) << p.shift );
        else if( p.format == VVR_OUT_PLANAR8 || p.format == VVR_OUT_NV12 ) out[i] = (uint8_t) sample( x );
        else if( ( x & 3 ) == 0 )
        {
          uint64_t g = 0;
          for( int k = 0; k < 4; k++ ) g |= (uint64_t) ( ( sample( x + k ) << p.shift ) & 0x3ff ) << ( 10 * k );
          for( int k = 0; k < 5; k++ ) out[i / 4 * 5 + k] = (uint8_t) ( g >> ( 8 * k ) );
        }
      }
    }
}

// ... and launch_output_narrow (k_output_narrow): the definition of vvr_set_output_narrowing (vvr.h) sample by sample, in 32 bits - the word as it
// lies, the constant of the cell at the sample's column and row in its own output plane (the Cb and the Cr of NV12's pair k: column k)
namespace {
uint8_t narrow_byte( uint32_t v, int i, int j, const NarrowArgs& na ) { return (uint8_t) std::min<uint32_t>( 255, ( v + ( i & 1 ? na.cell[j & 1] >> 16 : na.cell[j & 1] & 0xffff ) ) >> na.s ); }
}
void launch_output_narrow( hipStream_t, OutputFrameParams p, NarrowArgs na, void* dst )
{
  const bool semi = p.format == VVR_OUT_NV12;
  for( int c = 0; c < 3; c++ )
    for( int r = 0; r < ( p.w[c] ? p.h[c] : 0 ); r++ )
    {
      uint8_t* out = p.direct[c] ? p.direct[c] : (uint8_t*) dst + p.dstOff[c];
      for( int x = 0; x < p.w[c]; x++ )
      {
        const int k = semi && c == 1 ? 1 + ( x & 1 ) : c, col = semi && c == 1 ? x >> 1 : x;
        out[(size_t) r * p.w[c] + x] = narrow_byte( (uint16_t) p.src[k][(size_t) r * p.stride[k] + col], col, r, na );
      }
    }
}

// ... and launch_output_rgb (k_output_rgb): the definition of vvr.h sample by sample - positions, phases and taps from the table as launch_rescale
// takes them (step 16, add 0 / -8, shift 0, the chroma filter), the matrix, the transform, the stores of the planar and the interleaved formats
namespace {
uint16_t rgb_half_rne( float f )      // 0 or 1 / 65535 <= f <= 1: zero, a subnormal (below 2^-14: under a transform) or a normal half; round to nearest even (a carry out of the mantissa raises the exponent)
{
  uint32_t b; memcpy( &b, &f, 4 );
  if( !b ) return 0;
  const int e = (int) ( b >> 23 ) - 127;
  if( e < -14 )      // in units of 2^-24
  {
    const uint32_t man = ( b & 0x7fffff ) | 0x800000; const int sh = -e - 1;
    if( sh > 24 ) return 0;
    uint32_t q = man >> sh; const uint32_t rem = man & ( ( 1u << sh ) - 1 ), half = 1u << ( sh - 1 );
    if( rem > half || ( rem == half && ( q & 1 ) ) ) q++;
    return (uint16_t) q;
  }
  uint32_t h = (uint32_t) ( e + 15 ) << 10 | ( b & 0x7fffff ) >> 13;
  const uint32_t rem = b & 0x1fff;
  if( rem > 0x1000 || ( rem == 0x1000 && ( h & 1 ) ) ) h++;
  return (uint16_t) h;
}
}
static void rgb_region( const OutputRgbParams& p, void* dst );
void launch_output_rgb( hipStream_t, const OutputRgbParams& p, void* dst, const RgbRegions& rg )
{
  for( int z = 0; z < rg.count; z++ )
  {
    OutputRgbParams q = p;
    for( int c = 0; c < 3; c++ )
    {
      q.src[c] += ( rg.srcOff ? rg.srcOff[3 * z + c] : 0 ) + (size_t) z * rg.srcStep[c];
      if( q.direct[c] ) q.direct[c] += (size_t) z * rg.dstStep[c]; else q.dstOff[c] += (size_t) z * rg.dstStep[c];
    }
    rgb_region( q, dst );
  }
}
static void rgb_region( const OutputRgbParams& p, void* dst )
{
  const int cw = p.w / 2, ch = p.h / 2;
  std::vector<int> sums( (size_t) ch * p.w ), up[2];
  for( int pl = 0; pl < 2; pl++ )
  {
    const pel_t* src = p.src[1 + pl];
    up[pl].resize( (size_t) p.w * p.h );
    for( int i = 0; i < p.w; i++ )
    {
      const int refPos = 16 * i - ( p.collocated & 1 ? 0 : 8 ), integer = refPos >> 5, frac = refPos & 31;
      for( int j = 0; j < ch; j++ )
      {
        int sum = 0;
        for( int k = 0; k < 4; k++ ) sum += rescale_host_tbl::vvc_chroma_filter[frac][k] * src[(size_t) j * p.stride[1 + pl] + std::min( std::max( 0, integer + k - 1 ), cw - 1 )];
        sums[(size_t) j * p.w + i] = sum;
      }
    }
    for( int j = 0; j < p.h; j++ )
    {
      const int refPos = 16 * j - ( p.collocated & 2 ? 0 : 8 ), integer = refPos >> 5, frac = refPos & 31;
      for( int i = 0; i < p.w; i++ )
      {
        int sum = 0;
        for( int k = 0; k < 4; k++ ) sum += rescale_host_tbl::vvc_chroma_filter[frac][k] * sums[(size_t) std::min( std::max( 0, integer + k - 1 ), ch - 1 ) * p.w + i];
        up[pl][(size_t) j * p.w + i] = std::min( std::max( 0, ( sum + 2048 ) >> 12 ), p.maxVal );
      }
    }
  }
  for( int j = 0; j < p.h; j++ )
    for( int i = 0; i < p.w; i++ )
    {
      const size_t at = (size_t) j * p.w + i;
      const int y = p.src[0][(size_t) j * p.stride[0] + i] - p.yoff, u = up[0][at] - p.coff, v = up[1][at] - p.coff;
      const int rgb[3] = { ( p.cy * y + p.rv * v + 8192 ) >> 14, ( p.cy * y + p.gu * u + p.gv * v + 8192 ) >> 14, ( p.cy * y + p.bu * u + 8192 ) >> 14 };
      int L[3] = { 0, 0, 0 }, px[3] = { 0, 0, 0 }, E[3];
      for( int c = 0; c < 3 && p.xform; c++ ) L[c] = p.xform->lin[std::min( std::max( 0, rgb[c] ), p.maxOut )];      // (stage 1)
      for( int c = 0; c < 3; c++ )
      {
        E[c] = std::min( std::max( 0, rgb[c] ), p.maxOut );
        if( p.xform )
        {
          // stages 2 and 3 (vvr.h)
          const int64_t acc = (int64_t) p.xm[c][0] * L[0] + (int64_t) p.xm[c][1] * L[1] + (int64_t) p.xm[c][2] * L[2] + 8192;
          const int t = (int) std::min<int64_t>( std::max<int64_t>( 0, acc >> 14 ), 65535 ), i = t >> 6, f = t & 63;
          E[c] = ( p.xform->enc[i] * ( 64 - f ) + p.xform->enc[i + 1] * f + 32 ) >> 6;
        }
        else if( p.lut ) E[c] = ( E[c] * 65535 + ( p.maxOut >> 1 ) ) / p.maxOut;      // (the widening to the LUT's 16 bits)
      }
      if( p.lut )
      {
        // the 3-D LUT: the cell, the fractions in descending order, the four vertices of the tetrahedron (vvr.h)
        const int s = p.lutShift, S = 1 << s, n = p.lutN, step[3] = { 1, n, n * n };
        int idx[3], order[3] = { 0, 1, 2 }, f[3];
        for( int c = 0; c < 3; c++ ) { idx[c] = E[c] >> s; f[c] = E[c] & ( S - 1 ); }
        std::stable_sort( order, order + 3, [&]( int a, int b ) { return f[a] > f[b]; } );
        const int c0 = ( idx[2] * n + idx[1] ) * n + idx[0], c1 = c0 + step[order[0]], c2 = c1 + step[order[1]], c3 = c2 + step[order[2]];
        const int f1 = f[order[0]], f2 = f[order[1]], f3 = f[order[2]];
        for( int c = 0; c < 3; c++ )
          E[c] = ( p.lut[4 * c0 + c] * ( S - f1 ) + p.lut[4 * c1 + c] * ( f1 - f2 ) + p.lut[4 * c2 + c] * ( f2 - f3 ) + p.lut[4 * c3 + c] * f3 + ( S >> 1 ) ) >> s;
      }
      for( int c = 0; c < 3; c++ )
      {
        int val = E[c];
        // the 16 -> 8 and 16 -> 10 bit reductions under a transform or a LUT (vvr.h)
        if( ( p.xform || p.lut ) && ( p.format == VVR_OUT_RGB8 || p.format == VVR_OUT_RGBA8 || p.format == VVR_OUT_RGB24 ) ) val = ( val + 128 ) / 257;
        if( ( p.xform || p.lut ) && p.format == VVR_OUT_RGB10A2 ) val = ( val * 1023 + 32767 ) / 65535;
        px[c] = val;
        if( p.format >= VVR_OUT_RGBA8 ) continue;      // (one plane of pixels: below)
        uint8_t* out = p.direct[c] ? p.direct[c] : (uint8_t*) dst + p.dstOff[c];
        if( p.format == VVR_OUT_RGB8 ) out[at] = (uint8_t) val;
        else if( p.format == VVR_OUT_RGBF32 )
        {
          // two roundings: the product is a float32 of its own (volatile: no contraction into an FMA whatever the compiler's mode)
          volatile float t = (float) val * p.nscale[c];
          ( (float*) out )[at] = t + p.nbias[c];
        }
        else ( (uint16_t*) out )[at] = p.format == VVR_OUT_RGB16 ? (uint16_t) val : rgb_half_rne( (float) val * p.inv );
      }
      if( p.format < VVR_OUT_RGBA8 ) continue;
      // the interleaved formats: a pixel of the one plane in memory order (vvr.h); BGRA8 / BGR24 arrive as their class with swapRB set
      uint8_t* out = p.direct[0] ? p.direct[0] : (uint8_t*) dst + p.dstOff[0];
      const int r = p.swapRB ? px[2] : px[0], g = px[1], b = p.swapRB ? px[0] : px[2];
      if( p.format == VVR_OUT_RGBA8 )        { uint8_t* o = out + at * 4; o[0] = (uint8_t) r; o[1] = (uint8_t) g; o[2] = (uint8_t) b; o[3] = 255; }
      else if( p.format == VVR_OUT_RGB24 )   { uint8_t* o = out + at * 3; o[0] = (uint8_t) r; o[1] = (uint8_t) g; o[2] = (uint8_t) b; }
      else if( p.format == VVR_OUT_RGB10A2 ) { const uint32_t d = (uint32_t) r | (uint32_t) g << 10 | (uint32_t) b << 20 | 3u << 30; memcpy( out + at * 4, &d, 4 ); }
      else      // VVR_OUT_RGBA16F
      {
        const uint16_t hq[4] = { rgb_half_rne( (float) r * p.inv ), rgb_half_rne( (float) g * p.inv ), rgb_half_rne( (float) b * p.inv ), 0x3c00 };
        memcpy( out + at * 8, hq, 8 );
      }
    }
}

// ... and launch_output_yuv (k_output_yuv): the definition of vvr.h sample by sample - the two passes of launch_output_rgb above with the table's
// taps, the horizontal position 16 * i - ( 0 or 8 ) (4:4:4) or 32 * i (4:2:2: every phase is 0), then the sample, the word or the packed group
void launch_output_yuv( hipStream_t, const OutputYuvParams& p, void* dst )
{
  const int f = p.format;
  const bool full = f == VVR_OUT_YUV444P8 || f == VVR_OUT_YUV444P16 || f == VVR_OUT_Y410, bytes = f == VVR_OUT_YUV444P8 || f == VVR_OUT_YUV422P8;
  const int cw = p.w / 2, ch = p.h / 2, uw = full ? p.w : cw;      // (uw: the samples of a chroma row that leaves)
  std::vector<int> sums( (size_t) ch * uw ), up[2];
  for( int pl = 0; pl < 2; pl++ )
  {
    const pel_t* src = p.src[1 + pl];
    up[pl].resize( (size_t) uw * p.h );
    for( int i = 0; i < uw; i++ )
    {
      const int refPos = full ? 16 * i - ( p.collocated & 1 ? 0 : 8 ) : 32 * i, integer = refPos >> 5, frac = refPos & 31;
      for( int j = 0; j < ch; j++ )
      {
        int sum = 0;
        for( int k = 0; k < 4; k++ ) sum += rescale_host_tbl::vvc_chroma_filter[frac][k] * src[(size_t) j * p.stride[1 + pl] + std::min( std::max( 0, integer + k - 1 ), cw - 1 )];
        sums[(size_t) j * uw + i] = sum;
      }
    }
    for( int j = 0; j < p.h; j++ )
    {
      const int refPos = 16 * j - ( p.collocated & 2 ? 0 : 8 ), integer = refPos >> 5, frac = refPos & 31;
      for( int i = 0; i < uw; i++ )
      {
        int sum = 0;
        for( int k = 0; k < 4; k++ ) sum += rescale_host_tbl::vvc_chroma_filter[frac][k] * sums[(size_t) std::min( std::max( 0, integer + k - 1 ), ch - 1 ) * uw + i];
        up[pl][(size_t) j * uw + i] = std::min( std::max( 0, ( sum + 2048 ) >> 12 ), p.maxVal );
      }
    }
  }
  uint8_t* out[3];
  for( int c = 0; c < 3; c++ ) out[c] = p.direct[c] ? p.direct[c] : (uint8_t*) dst + p.dstOff[c];
  auto luma = [&]( int i, int j ) { return (uint32_t) (uint16_t) p.src[0][(size_t) j * p.stride[0] + i]; };
  const size_t v210Row = (size_t) ( p.w + 5 ) / 6 * 16;
  for( int j = 0; j < p.h; j++ )
  {
    if( f == VVR_OUT_V210 ) memset( out[0] + j * v210Row, 0, v210Row );      // (the fields of pixels that do not exist)
    for( int i = 0; i < p.w; i++ )
    {
      uint32_t y = luma( i, j ) << p.shift, u = (uint32_t) up[0][(size_t) j * uw + ( full ? i : i / 2 )] << p.shift, v = (uint32_t) up[1][(size_t) j * uw + ( full ? i : i / 2 )] << p.shift;
      if( p.narrow.s )      // (the byte formats in a context of 9 or 10 bits: the chroma at its own column - of the pixel pair at 4:2:2)
      {
        const int ci = full ? i : i / 2;
        y = narrow_byte( y, i, j, p.narrow ); u = narrow_byte( u, ci, j, p.narrow ); v = narrow_byte( v, ci, j, p.narrow );
      }
      const size_t at = (size_t) j * p.w + i, cat = (size_t) j * uw + i / 2;
      switch( f )
      {
      case VVR_OUT_YUV444P8: case VVR_OUT_YUV422P8:
        out[0][at] = (uint8_t) y;
        if( full ) { out[1][at] = (uint8_t) u; out[2][at] = (uint8_t) v; } else if( !( i & 1 ) ) { out[1][cat] = (uint8_t) u; out[2][cat] = (uint8_t) v; }
        break;
      case VVR_OUT_YUV444P16: case VVR_OUT_YUV422P16:
        ( (uint16_t*) out[0] )[at] = (uint16_t) y;
        if( full ) { ( (uint16_t*) out[1] )[at] = (uint16_t) u; ( (uint16_t*) out[2] )[at] = (uint16_t) v; } else if( !( i & 1 ) ) { ( (uint16_t*) out[1] )[cat] = (uint16_t) u; ( (uint16_t*) out[2] )[cat] = (uint16_t) v; }
        break;
      case VVR_OUT_UYVY: out[0][2 * at + 1] = (uint8_t) y; if( !( i & 1 ) ) { out[0][2 * at] = (uint8_t) u; out[0][2 * at + 2] = (uint8_t) v; } break;
      case VVR_OUT_YUY2: out[0][2 * at] = (uint8_t) y; if( !( i & 1 ) ) { out[0][2 * at + 1] = (uint8_t) u; out[0][2 * at + 3] = (uint8_t) v; } break;
      case VVR_OUT_Y210: ( (uint16_t*) out[0] )[2 * at] = (uint16_t) y; if( !( i & 1 ) ) { ( (uint16_t*) out[0] )[2 * at + 1] = (uint16_t) u; ( (uint16_t*) out[0] )[2 * at + 3] = (uint16_t) v; } break;
      case VVR_OUT_Y410: { const uint32_t d = u | y << 10 | v << 20 | 3u << 30; memcpy( out[0] + at * 4, &d, 4 ); } break;
      default:      // VVR_OUT_V210: the 10-bit fields of a group in order Cb0 Y0 Cr0 | Y1 Cb1 Y2 | Cr1 Y3 Cb2 | Y4 Cr2 Y5, three to a dword
      {
        uint32_t* g = (uint32_t*) ( out[0] + j * v210Row ) + i / 6 * 4;
        static const int yField[6] = { 1, 3, 5, 7, 9, 11 }, uField[3] = { 0, 4, 8 }, vField[3] = { 2, 6, 10 };
        const int k = i % 6;
        g[yField[k] / 3] |= y << ( 10 * ( yField[k] % 3 ) );
        if( !( k & 1 ) ) { g[uField[k / 2] / 3] |= u << ( 10 * ( uField[k / 2] % 3 ) ); g[vField[k / 2] / 3] |= v << ( 10 * ( vField[k / 2] % 3 ) ); }
      }
      }
    }
  }
}

// ... and launch_hash_rows / launch_hash_combine (k_hash_rows, k_hash_combine): per row the CRC register reached from 0 bit by bit (compCRC,
// PicYuvMD5.cpp:99-137) or the checksum share (compChecksum, :152-176); the rows chained with the request's power of x, or added
void launch_hash_rows( hipStream_t, const HashParams& p, uint32_t* rows )
{
  for( int c = 0; c < p.numComp; c++ )
  {
    for( int y = 0; y < p.h[c]; y++ )
    {
      uint32_t acc = 0;
      for( int x = 0; x < p.w[c]; x++ )
      {
        const uint32_t v = (uint16_t) p.src[c][(size_t) y * p.stride[c] + x];
        if( !p.crc ) { const uint32_t mask = ( ( x & 0xff ) ^ ( y & 0xff ) ^ ( x >> 8 ) ^ ( y >> 8 ) ) & 0xff; acc += ( v & 0xff ) ^ mask; if( p.two ) acc += ( v >> 8 ) ^ mask; }
        else for( int b = 0; b < ( p.two ? 2 : 1 ); b++ ) for( int bit = 7; bit >= 0; bit-- )
        {
          const uint32_t byte = b ? v >> 8 : v & 0xff, msb = ( acc >> 15 ) & 1;
          acc = ( ( ( acc << 1 ) + ( ( byte >> bit ) & 1 ) ) & 0xffff ) ^ ( msb * 0x1021 );
        }
      }
      rows[y] = acc;
    }
    rows += p.h[c];
  }
}
void launch_hash_combine( hipStream_t, const HashParams& p, const uint32_t* rows, uint32_t* out )
{
  for( int c = 0; c < p.numComp; c++ )
  {
    uint32_t acc = p.crc ? 0xffff : 0;
    for( int r = 0; r < p.h[c]; r++ ) acc = p.crc ? crcMul( acc, p.xRowTree[c][0] ) ^ ( rows[r] & 0xffff ) : acc + rows[r];
    out[c] = p.crc ? crcMul( acc, 0x1021 ) : acc;
    rows += p.h[c];
  }
}

// ... and launch_output_stats / launch_output_stats_sum (k_output_stats, the statistics class of k_output_rgb, k_output_stats_sum): the definition
// of vvr.h sample by sample - the luma as it lies there, R, G, B as launch_output_rgb above stores them for VVR_OUT_RGB16 at od = bd with no
// transform and no LUT - counted into the first copy of the words; the copies folded
void launch_output_stats( hipStream_t, const OutputRgbParams& p, int rgb, uint32_t* shards )
{
  for( int j = 0; j < p.h; j++ )
    for( int i = 0; i < p.w; i++ ) shards[std::min<int>( (uint16_t) p.src[0][(size_t) j * p.stride[0] + i], 1023 )]++;
  if( !rgb ) return;
  const size_t count = (size_t) p.w * p.h;
  std::vector<uint16_t> planes( 3 * count );
  OutputRgbParams q = p;
  q.format = VVR_OUT_RGB16; q.xform = nullptr; q.lut = nullptr; q.lutN = 0;
  for( int k = 0; k < 3; k++ ) { q.direct[k] = nullptr; q.dstOff[k] = k * count * sizeof( uint16_t ); }
  launch_output_rgb( nullptr, q, planes.data() );
  for( size_t at = 0; at < count; at++ )
  {
    uint32_t top = 0;
    for( int k = 0; k < 3; k++ )
    {
      const uint32_t v = planes[k * count + at];
      top = std::max( top, v );
      shards[2048 + k] = std::max( shards[2048 + k], v ); shards[2051 + k] = std::max( shards[2051 + k], (uint32_t) p.maxVal - v );
    }
    shards[1024 + top]++;
  }
}
void launch_output_stats_sum( hipStream_t, const uint32_t* shards, uint32_t* out )
{
  for( int i = 0; i < STATS_WORDS; i++ )
  {
    uint32_t acc = 0;
    for( int k = 0; k < STATS_SHARDS; k++ ) { const uint32_t v = shards[(size_t) k * STATS_WORDS + i]; acc = i < 2048 ? acc + v : std::max( acc, v ); }
    out[i] = acc;
  }
}

// ... and launch_output_compare / launch_output_compare_sum (k_output_compare, k_output_compare_sum): the definition of vvr.h sample by sample, a
// record per block and component as vvr_device.h lays them out; the records folded
void launch_output_compare( hipStream_t, const CompareParams& p, uint32_t* recs, uint32_t* map )
{
  const int blocks = p.nbx * p.nby;
  for( int b = 0; b < blocks; b++ )
  {
    map[b] = 0;
    for( int c = 0; c < p.numComp; c++ )
    {
      const int side = c ? 32 : 64, i0 = ( b % p.nbx ) * side, j0 = ( b / p.nbx ) * side;
      uint64_t sse = 0; uint32_t sad = 0, count = 0, top = 0, first = 0xffffffffu;
      for( int j = j0; j < std::min( j0 + side, p.h[c] ); j++ )
        for( int i = i0; i < std::min( i0 + side, p.w[c] ); i++ )
        {
          const uint8_t* r = p.ref[c] + (size_t) j * p.refStride[c] + (size_t) i * p.refBytes;
          const int32_t d = (int32_t) (uint16_t) p.src[c][(size_t) j * p.stride[c] + i] - (int32_t) ( p.refBytes == 1 ? r[0] : r[0] | r[1] << 8 );
          if( !d ) continue;
          const uint32_t a = (uint32_t) std::abs( d );
          sse += (uint64_t) a * a; sad += a; count++; top = std::max( top, a ); first = std::min( first, (uint32_t) ( j * p.w[c] + i ) );
        }
      uint32_t* rec = recs + ( (size_t) c * blocks + b ) * CMP_REC_WORDS;
      rec[0] = (uint32_t) sse; rec[1] = (uint32_t) ( sse >> 32 ); rec[2] = sad; rec[3] = count; rec[4] = top; rec[5] = first;
      map[b] += count;
    }
  }
}
// ... and launch_output_compare_scaled (k_output_compare_scaled) as what it stands for: every component rescaled by the loop above, then the
// comparison's loop over the rescaled planes
void launch_output_compare_scaled( hipStream_t s, CompareScaledParams q, uint32_t* recs, uint32_t* map )
{
  std::vector<uint16_t> planes[3];
  CompareParams p; memset( &p, 0, sizeof( p ) );
  for( int k = 0; k < q.numComp; k++ )
  {
    RescaleParams r = q.rs[k]; r.bytesPerSample = 2;
    planes[k].resize( (size_t) r.outW * r.outH );
    launch_rescale( s, r, planes[k].data() );
    p.src[k] = (const pel_t*) planes[k].data(); p.stride[k] = r.outW; p.w[k] = r.outW; p.h[k] = r.outH; p.ref[k] = q.ref[k]; p.refStride[k] = q.refStride[k];
  }
  p.numComp = q.numComp; p.refBytes = q.refBytes; p.nbx = q.nbx; p.nby = q.nby; p.bySample = 1;
  launch_output_compare( s, p, recs, map );
}
void launch_output_compare_sum( hipStream_t, const uint32_t* recs, int blocks, int numComp, uint32_t* out )
{
  for( int c = 0; c < numComp; c++ )
  {
    uint64_t sse = 0, sad = 0, count = 0; uint32_t top = 0, first = 0xffffffffu;
    for( int b = 0; b < blocks; b++ )
    {
      const uint32_t* rec = recs + ( (size_t) c * blocks + b ) * CMP_REC_WORDS;
      sse += rec[0] | (uint64_t) rec[1] << 32; sad += rec[2]; count += rec[3]; top = std::max( top, rec[4] ); first = std::min( first, rec[5] );
    }
    uint32_t* o = out + c * CMP_OUT_WORDS;
    o[0] = (uint32_t) sse; o[1] = (uint32_t) ( sse >> 32 ); o[2] = (uint32_t) sad; o[3] = (uint32_t) ( sad >> 32 ); o[4] = (uint32_t) count; o[5] = (uint32_t) ( count >> 32 );
    o[6] = top; o[7] = first;
  }
}

// ... and launch_output_ssim / launch_output_ssim_sum (k_output_ssim, k_output_ssim_sum): the definition of vvr.h window by window and sample by
// sample, a record per block and component as vvr_device.h lays them out; the records folded
void launch_output_ssim( hipStream_t, const CompareParams& p, int bitDepth, uint32_t* recs, int32_t* map )
{
  const int blocks = p.nbx * p.nby;
  const int64_t L = ( 1 << bitDepth ) - 1, N = 64, C1 = ( L * L * 4096 + 5000 ) / 10000, C2 = ( 9 * L * L * 4096 + 5000 ) / 10000;
  for( int b = 0; b < blocks; b++ )
  {
    map[b] = 0x7fffffff;
    for( int c = 0; c < p.numComp; c++ )
    {
      const int side = c ? 32 : 64, i0 = ( b % p.nbx ) * side, j0 = ( b / p.nbx ) * side, windowsX = p.w[c] >= 8 ? ( p.w[c] - 8 ) / 4 + 1 : 0;
      int64_t sum = 0; uint64_t key = SSIM_NO_WINDOW;
      for( int j = j0; j < j0 + side && j + 8 <= p.h[c]; j += 4 )
        for( int i = i0; i < i0 + side && i + 8 <= p.w[c]; i += 4 )
        {
          int64_t s1 = 0, s2 = 0, sxx = 0, syy = 0, sxy = 0;
          for( int jj = j; jj < j + 8; jj++ )
            for( int ii = i; ii < i + 8; ii++ )
            {
              const uint8_t* r = p.ref[c] + (size_t) jj * p.refStride[c] + (size_t) ii * p.refBytes;
              const int64_t x = std::min<int64_t>( (uint16_t) p.src[c][(size_t) jj * p.stride[c] + ii], L ), y = std::min<int64_t>( p.refBytes == 1 ? r[0] : r[0] | r[1] << 8, L );
              s1 += x; s2 += y; sxx += x * x; syy += y * y; sxy += x * y;
            }
          const int64_t A1 = 2 * s1 * s2 + C1, B1 = s1 * s1 + s2 * s2 + C1, A2 = 2 * ( N * sxy - s1 * s2 ) + C2, B2 = ( N * sxx - s1 * s1 ) + ( N * syy - s2 * s2 ) + C2;
          const int64_t l = ( A1 * 16777216 ) / B1, cs = ( A2 * 16777216 ) / B2, v = ( l * cs ) / 16777216;
          sum += v;
          key = std::min( key, (uint64_t) ( (uint32_t) (int32_t) v ^ 0x80000000u ) << 32 | (uint32_t) ( ( j / 4 ) * windowsX + i / 4 ) );
        }
      uint32_t* rec = recs + ( (size_t) c * blocks + b ) * SSIM_REC_WORDS;
      rec[0] = (uint32_t) (uint64_t) sum; rec[1] = (uint32_t) ( (uint64_t) sum >> 32 ); rec[2] = (uint32_t) key; rec[3] = (uint32_t) ( key >> 32 );
      map[b] = std::min( map[b], (int32_t) ( (uint32_t) ( key >> 32 ) ^ 0x80000000u ) );
    }
  }
}
void launch_output_ssim_sum( hipStream_t, const uint32_t* recs, int blocks, int numComp, uint32_t* out )
{
  for( int c = 0; c < numComp; c++ )
  {
    uint64_t sum = 0, key = SSIM_NO_WINDOW;      // (the sum in two's complement)
    for( int b = 0; b < blocks; b++ )
    {
      const uint32_t* rec = recs + ( (size_t) c * blocks + b ) * SSIM_REC_WORDS;
      sum += rec[0] | (uint64_t) rec[1] << 32; key = std::min( key, rec[2] | (uint64_t) rec[3] << 32 );
    }
    uint32_t* o = out + c * SSIM_OUT_WORDS;
    o[0] = (uint32_t) sum; o[1] = (uint32_t) ( sum >> 32 ); o[2] = (uint32_t) key; o[3] = (uint32_t) ( key >> 32 );
  }
}

// ... and launch_output_msssim / launch_output_msssim_sum (k_output_msssim, k_output_msssim_sum): one level of the definition of vvr.h window by
// window and sample by sample, a record per block and component as vvr_device.h lays them out; with `next` the whole next level, every sample
// ( i, j ) with i < w >> 1 and j < h >> 1 as the rounded mean of the 2 x 2 clamped samples above it; the records of all levels folded
void launch_output_msssim( hipStream_t, const CompareParams& p, int bitDepth, uint32_t* recs, const MsssimNext* next )
{
  const int blocks = p.nbx * p.nby;
  const int64_t L = ( 1 << bitDepth ) - 1, N = 64, C1 = ( L * L * 4096 + 5000 ) / 10000, C2 = ( 9 * L * L * 4096 + 5000 ) / 10000;
  auto sampleX = [&]( int c, int i, int j ) { return std::min<int64_t>( (uint16_t) p.src[c][(size_t) j * p.stride[c] + i], L ); };
  auto sampleY = [&]( int c, int i, int j ) { const uint8_t* r = p.ref[c] + (size_t) j * p.refStride[c] + (size_t) i * p.refBytes; return std::min<int64_t>( p.refBytes == 1 ? r[0] : r[0] | r[1] << 8, L ); };
  for( int c = 0; c < p.numComp; c++ )
  {
    for( int b = 0; b < blocks; b++ )
    {
      const int side = c ? 32 : 64, i0 = ( b % p.nbx ) * side, j0 = ( b / p.nbx ) * side;
      int64_t sumCs = 0, sumV = 0;
      for( int j = j0; j < j0 + side && j + 8 <= p.h[c]; j += 4 )
        for( int i = i0; i < i0 + side && i + 8 <= p.w[c]; i += 4 )
        {
          int64_t s1 = 0, s2 = 0, sxx = 0, syy = 0, sxy = 0;
          for( int jj = j; jj < j + 8; jj++ )
            for( int ii = i; ii < i + 8; ii++ )
            {
              const int64_t x = sampleX( c, ii, jj ), y = sampleY( c, ii, jj );
              s1 += x; s2 += y; sxx += x * x; syy += y * y; sxy += x * y;
            }
          const int64_t A1 = 2 * s1 * s2 + C1, B1 = s1 * s1 + s2 * s2 + C1, A2 = 2 * ( N * sxy - s1 * s2 ) + C2, B2 = ( N * sxx - s1 * s1 ) + ( N * syy - s2 * s2 ) + C2;
          const int64_t l = ( A1 * 16777216 ) / B1, cs = ( A2 * 16777216 ) / B2, v = ( l * cs ) / 16777216;
          sumCs += cs; sumV += v;
        }
      uint32_t* rec = recs + ( (size_t) c * blocks + b ) * MSSSIM_REC_WORDS;
      rec[0] = (uint32_t) (uint64_t) sumCs; rec[1] = (uint32_t) ( (uint64_t) sumCs >> 32 ); rec[2] = (uint32_t) (uint64_t) sumV; rec[3] = (uint32_t) ( (uint64_t) sumV >> 32 );
    }
    for( int j = 0; next && j < p.h[c] >> 1; j++ )
      for( int i = 0; i < p.w[c] >> 1; i++ )
      {
        next->x[c][(size_t) j * next->stride[c] + i] = (uint16_t) ( ( sampleX( c, 2 * i, 2 * j ) + sampleX( c, 2 * i + 1, 2 * j ) + sampleX( c, 2 * i, 2 * j + 1 ) + sampleX( c, 2 * i + 1, 2 * j + 1 ) + 2 ) >> 2 );
        next->y[c][(size_t) j * next->stride[c] + i] = (uint16_t) ( ( sampleY( c, 2 * i, 2 * j ) + sampleY( c, 2 * i + 1, 2 * j ) + sampleY( c, 2 * i, 2 * j + 1 ) + sampleY( c, 2 * i + 1, 2 * j + 1 ) + 2 ) >> 2 );
      }
  }
}
void launch_output_msssim_sum( hipStream_t, const uint32_t* recs, const MsssimFold& f, int numComp, uint32_t* out )
{
  for( int k = 0; k < f.scales; k++ )
    for( int c = 0; c < numComp; c++ )
    {
      uint64_t cs = 0, v = 0;      // (two's complement)
      for( int b = 0; b < f.blocks[k]; b++ )
      {
        const uint32_t* rec = recs + f.recOff[k] + ( (size_t) c * f.blocks[k] + b ) * MSSSIM_REC_WORDS;
        cs += rec[0] | (uint64_t) rec[1] << 32; v += rec[2] | (uint64_t) rec[3] << 32;
      }
      uint32_t* o = out + ( k * numComp + c ) * MSSSIM_OUT_WORDS;
      o[0] = (uint32_t) cs; o[1] = (uint32_t) ( cs >> 32 ); o[2] = (uint32_t) v; o[3] = (uint32_t) ( v >> 32 );
    }
}

// ... and launch_output_xpsnr (k_output_xpsnr): the definition of vvr.h sample by sample and position by position, every squared difference and
// every position added to the record of the block that holds it; the weights of filter 2 as the table vvr.h prints
void launch_output_xpsnr( hipStream_t, const XpsnrParams& P, unsigned long long* recs )
{
  static const int W2[6][6] = { { 0, -1, -1, -1, -1, 0 }, { -1, -2, -3, -3, -2, -1 }, { -1, -3, 12, 12, -3, -1 }, { -1, -3, 12, 12, -3, -1 }, { -1, -2, -3, -3, -2, -1 }, { 0, -1, -1, -1, -1, 0 } };
  const CompareParams& p = P.c;
  const int B = P.block, w = p.w[0], h = p.h[0];
  auto sample = [&]( const uint8_t* base, size_t stride, int i, int j ) { const uint8_t* r = base + (size_t) j * stride + (size_t) i * p.refBytes; return (int64_t) ( p.refBytes == 1 ? r[0] : r[0] | r[1] << 8 ); };
  auto o = [&]( int i, int j ) { return sample( p.ref[0], p.refStride[0], i, j ); };
  auto o1 = [&]( int i, int j ) { return sample( P.prev[0], P.prevStride[0], i, j ); };
  auto o2 = [&]( int i, int j ) { return sample( P.prev[1], P.prevStride[1], i, j ); };
  for( int c = 0; c < p.numComp; c++ )
    for( int j = 0; j < p.h[c]; j++ )
      for( int i = 0; i < p.w[c]; i++ )
      {
        const int sh = c ? 1 : 0;
        const int64_t d = (int64_t) (uint16_t) p.src[c][(size_t) j * p.stride[c] + i] - sample( p.ref[c], p.refStride[c], i, j );
        recs[( (size_t) ( ( j << sh ) / B ) * P.blocksX + ( i << sh ) / B ) * XPSNR_REC_WORDS + c] += (uint64_t) ( d * d );
      }
  const int step = P.filter == 2 ? 2 : 1, first = P.filter == 2 ? 2 : 1, lastX = P.filter == 2 ? w - 4 : w - 2, lastY = P.filter == 2 ? h - 4 : h - 2;
  for( int j = first; j <= lastY; j += step )
    for( int i = first; i <= lastX; i += step )
    {
      int64_t f = 0, t = 0;
      if( P.filter == 1 )
      {
        f = 12 * o( i, j ) - 2 * ( o( i - 1, j ) + o( i + 1, j ) + o( i, j - 1 ) + o( i, j + 1 ) ) - ( o( i - 1, j - 1 ) + o( i + 1, j - 1 ) + o( i - 1, j + 1 ) + o( i + 1, j + 1 ) );
        if( P.temporal == 1 ) t = o( i, j ) - o1( i, j );
        if( P.temporal == 2 ) t = o( i, j ) - 2 * o1( i, j ) + o2( i, j );
      }
      else
      {
        for( int dj = 0; dj < 6; dj++ )
          for( int di = 0; di < 6; di++ ) f += W2[dj][di] * o( i - 2 + di, j - 2 + dj );
        auto S = [&]( auto& a ) { return a( i, j ) + a( i + 1, j ) + a( i, j + 1 ) + a( i + 1, j + 1 ); };
        if( P.temporal == 1 ) t = S( o ) - S( o1 );
        if( P.temporal == 2 ) t = S( o ) - 2 * S( o1 ) + S( o2 );
      }
      unsigned long long* rec = recs + ( (size_t) ( j / B ) * P.blocksX + i / B ) * XPSNR_REC_WORDS;
      rec[3] += (uint64_t) ( f < 0 ? -f : f ); rec[4] += (uint64_t) ( t < 0 ? -t : t ); rec[5] += 1;
    }
}
// the geometry k_output_compare_scaled is launched with (compare_scaled_geometry, vvr_device.h) for a window of w x h luma samples rescaled to
// outW x outH, for the host tests: out[0 .. 14] = tileH[3], rowsCap[3], tilesX[3], first[4], the bytes of dynamic LDS, the words cleared
extern "C" __attribute__(( visibility( "default" ) )) void vvt_compare_scaled_geometry( int w, int h, int outW, int outH, int numComp, long long* out )
{
  CompareScaledParams p; memset( &p, 0, sizeof( p ) );
  p.numComp = numComp; p.nbx = ( outW + 63 ) / 64; p.nby = ( outH + 63 ) / 64;
  for( int k = 0; k < numComp; k++ )
  {
    const int cs = k ? 1 : 0, fracShift = k ? 5 : 4;
    RescaleParams& r = p.rs[k];
    r.w = w >> cs; r.h = h >> cs; r.outW = outW >> cs; r.outH = outH >> cs; r.luma = k == 0;
    int scale;
    rescale_axis( r.w, r.outW, cs, 1, fracShift, scale, r.addX, r.shiftX ); r.stepX = scale << cs;
    rescale_axis( r.h, r.outH, cs, 1, fracShift, scale, r.addY, r.shiftY ); r.stepY = scale << cs;
  }
  const CompareScaledGeometry g = compare_scaled_geometry( p );
  for( int k = 0; k < 3; k++ ) { out[k] = p.tileH[k]; out[3 + k] = p.rowsCap[k]; out[6 + k] = p.tilesX[k]; }
  for( int k = 0; k < 4; k++ ) out[9 + k] = p.first[k];
  out[13] = (long long) g.ldsBytes; out[14] = (long long) g.clearWords;
}
#endif

extern "C" {

VVR_API int vvr_read_output( vvr_context* c, int slot, int comp, int x, int y, int w, int h, int bytesPerSample, void* dst, size_t dstStrideBytes )
{
  if( !c || slot < 0 || slot >= (int) c->slots.size() || comp < 0 || comp > 2 || !c->slots[slot].p[comp] || !dst ) return VVR_ERR_PARAMETER;
  const DevPlanes& d = c->slots[slot];
  if( x < 0 || y < 0 || w <= 0 || h <= 0 || x + w > d.w[comp] || y + h > d.h[comp] || ( bytesPerSample != 1 && bytesPerSample != 2 ) || dstStrideBytes < (size_t) w * bytesPerSample )
  { c->setError( "vvr_read_output: window outside the plane, bad sample size or stride" ); return VVR_ERR_PARAMETER; }
  if( bytesPerSample == 1 && c->cfg.bit_depth > 8 ) { c->setError( "vvr_read_output: 8-bit output of a stream with more than 8 bits per sample (only narrowing of 8-bit content, vvdecimpl.cpp:853)" ); return VVR_ERR_PARAMETER; }
  hipSetDevice( c->device );
  int rc = vvr_sync( c ); if( rc != VVR_OK ) return rc;
  // the window is packed on the device (rows back to back, 1 or 2 bytes per sample), crosses PCIe as one copy into pinned memory and is laid
  // out with the caller's stride from there
  const size_t rowBytes = (size_t) w * bytesPerSample, bytes = alignUp( rowBytes * h, 256 );
  if( ( rc = ensureOutputScratch( c, bytes, bytes ) ) != VVR_OK ) return rc;
  hipStream_t s = c->streams[0];
  launch_output_window( s, d.p[comp] + (size_t) y * d.stride[comp] + x, d.stride[comp], w, h, bytesPerSample, c->outDev );
  HIPCHK( c, hipGetLastError() );
  HIPCHK( c, hipMemcpyAsync( c->outHost, c->outDev, rowBytes * h, hipMemcpyDeviceToHost, s ) );
  HIPCHK( c, hipStreamSynchronize( s ) );
  for( int r = 0; r < h; r++ ) memcpy( (uint8_t*) dst + (size_t) r * dstStrideBytes, (const uint8_t*) c->outHost + (size_t) r * rowBytes, rowBytes );
  return VVR_OK;
}

VVR_API int vvr_read_output_scaled( vvr_context* c, int slot, int comp, int x, int y, int w, int h, int outW, int outH, int collocated, int bytesPerSample, void* dst, size_t dstStrideBytes )
{
  if( !c || slot < 0 || slot >= (int) c->slots.size() || comp < 0 || comp > 2 || !c->slots[slot].p[comp] || !dst ) return VVR_ERR_PARAMETER;
  const DevPlanes d = pictureIn( c, slot );      // (the picture in the slot: an RPR picture is smaller than the slot)
  if( x < 0 || y < 0 || w <= 0 || h <= 0 || x + w > d.w[comp] || y + h > d.h[comp] || ( bytesPerSample != 1 && bytesPerSample != 2 ) )
  { c->setError( "vvr_read_output_scaled: window outside the picture's plane or bad sample size" ); return VVR_ERR_PARAMETER; }
  if( outW <= 0 || outH <= 0 || outW > 8192 || outH > 8192 || w > 8 * outW || h > 8 * outH || outW > 8 * w || outH > 8 * h )
  { c->setError( "vvr_read_output_scaled: output sides must be 1..8192 and within 1/8 .. 8 times the window's" ); return VVR_ERR_PARAMETER; }
  if( dstStrideBytes < (size_t) outW * bytesPerSample ) { c->setError( "vvr_read_output_scaled: stride below the output's row" ); return VVR_ERR_PARAMETER; }
  if( bytesPerSample == 1 && c->cfg.bit_depth > 8 ) { c->setError( "vvr_read_output_scaled: 8-bit output of a stream with more than 8 bits per sample (only narrowing of 8-bit content, vvdecimpl.cpp:853)" ); return VVR_ERR_PARAMETER; }
  hipSetDevice( c->device );
  int rc = vvr_sync( c ); if( rc != VVR_OK ) return rc;
  // packed on the device, one copy into pinned memory, rows at the caller's stride from there (as vvr_read_output)
  const size_t rowBytes = (size_t) outW * bytesPerSample, bytes = alignUp( rowBytes * outH, 256 );
  if( ( rc = ensureOutputScratch( c, bytes, bytes ) ) != VVR_OK ) return rc;
  hipStream_t s = c->streams[0];
  const pel_t* src = d.p[comp] + (size_t) y * d.stride[comp] + x;
  if( w == outW && h == outH )
    launch_output_window( s, src, d.stride[comp], w, h, bytesPerSample, c->outDev );       // the reference copies (Buffer.cpp:243)
  else
  {
    // the component's subsampling: 4:2:0 chroma is half size both ways; luma is always collocated (vvdecimpl.cpp:1651)
    const bool luma = comp == 0;
    const int cs = luma ? 0 : 1, colX = luma ? 1 : collocated & 1, colY = luma ? 1 : ( collocated >> 1 ) & 1, fracShift = luma ? 4 : 5;
    RescaleParams p;
    p.src = src; p.stride = d.stride[comp]; p.w = w; p.h = h; p.outW = outW; p.outH = outH;
    p.luma = luma; p.maxVal = ( 1 << c->cfg.bit_depth ) - 1; p.bytesPerSample = bytesPerSample;
    int scale;
    rescale_axis( w, outW, cs, colX, fracShift, scale, p.addX, p.shiftX ); p.stepX = scale << cs;
    rescale_axis( h, outH, cs, colY, fracShift, scale, p.addY, p.shiftY ); p.stepY = scale << cs;
    launch_rescale( s, p, c->outDev );
  }
  HIPCHK( c, hipGetLastError() );
  HIPCHK( c, hipMemcpyAsync( c->outHost, c->outDev, rowBytes * outH, hipMemcpyDeviceToHost, s ) );
  HIPCHK( c, hipStreamSynchronize( s ) );
  for( int r = 0; r < outH; r++ ) memcpy( (uint8_t*) dst + (size_t) r * dstStrideBytes, (const uint8_t*) c->outHost + (size_t) r * rowBytes, rowBytes );
  return VVR_OK;
}

VVR_API int vvr_set_film_grain( vvr_context* c, const vvr_film_grain_bank* bank )
{
  if( !c ) return VVR_ERR_PARAMETER;
  if( !bank ) { c->grainBank.reset(); return VVR_OK; }
  if( bank->struct_size != sizeof( vvr_film_grain_bank ) ) { c->setError( "vvr_set_film_grain: struct_size is not sizeof( vvr_film_grain_bank )" ); return VVR_ERR_PARAMETER; }
  if( bank->shift < 2 || bank->shift > 7 ) { c->setError( "vvr_set_film_grain: shift outside 2..7" ); return VVR_ERR_PARAMETER; }
  for( int k = 0; k < 3; k++ )
    for( int i = 0; i < 256; i++ )
      if( bank->pattern_lut[k][i] >= 0x80 ) { c->setError( "vvr_set_film_grain: pattern_lut entry >= 0x80 (8 patterns)" ); return VVR_ERR_PARAMETER; }
  if( !c->grainBank ) c->grainBank.reset( new vvr_film_grain_bank );
  *c->grainBank = *bank;
  c->grainBankStale = true;
  return VVR_OK;
}

VVR_API int vvr_set_film_grain_seed( vvr_context* c, uint32_t seed )
{
  if( !c ) return VVR_ERR_PARAMETER;
  c->grainSeed = seed;
  return VVR_OK;
}

VVR_API int vvr_set_output_colour( vvr_context* c, int matrixCoefficients, int fullRange )
{
  if( !c ) return VVR_ERR_PARAMETER;
  std::lock_guard<std::mutex> lk( c->mu );
  double kr, kb;
  if( !rgb_matrix( matrixCoefficients, kr, kb ) ) { c->setError( "vvr_set_output_colour: matrix_coefficients must be 1 (BT.709), 5 or 6 (BT.601) or 9 (BT.2020 non-constant luminance)" ); return VVR_ERR_PARAMETER; }
  if( fullRange != 0 && fullRange != 1 ) { c->setError( "vvr_set_output_colour: full_range must be 0 or 1" ); return VVR_ERR_PARAMETER; }
  c->outMatrix = matrixCoefficients; c->outFullRange = fullRange;
  return VVR_OK;
}

VVR_API int vvr_set_output_normalisation( vvr_context* c, const float mean[3], const float stdDev[3] )
{
  if( !c ) return VVR_ERR_PARAMETER;
  std::lock_guard<std::mutex> lk( c->mu );
  if( !mean && !stdDev ) { c->outNorm = false; return VVR_OK; }
  if( !mean || !stdDev ) { c->setError( "vvr_set_output_normalisation: mean and std are given together, or both NULL" ); return VVR_ERR_PARAMETER; }
  const float lim = 1048576.f;      // 2^20
  for( int k = 0; k < 3; k++ )
  {
    if( !std::isfinite( mean[k] ) || !std::isfinite( stdDev[k] ) ) { c->setError( "vvr_set_output_normalisation: an entry is not finite" ); return VVR_ERR_PARAMETER; }
    if( stdDev[k] < 1 / lim || stdDev[k] > lim ) { c->setError( "vvr_set_output_normalisation: std outside [ 2^-20, 2^20 ]" ); return VVR_ERR_PARAMETER; }
    if( std::fabs( mean[k] ) > lim ) { c->setError( "vvr_set_output_normalisation: | mean | above 2^20" ); return VVR_ERR_PARAMETER; }
  }
  for( int k = 0; k < 3; k++ ) { c->outMean[k] = mean[k]; c->outStd[k] = stdDev[k]; }
  c->outNorm = true;
  return VVR_OK;
}

VVR_API int vvr_set_output_transform( vvr_context* c, const vvr_output_transform* t )
{
  if( !c ) return VVR_ERR_PARAMETER;
  std::lock_guard<std::mutex> lk( c->mu );
  if( !t ) { c->xform.reset(); return VVR_OK; }
  if( t->struct_size != sizeof( vvr_output_transform ) ) { c->setError( "vvr_set_output_transform: struct_size is not sizeof( vvr_output_transform )" ); return VVR_ERR_PARAMETER; }
  for( int k = 0; k < 3; k++ )
    for( int j = 0; j < 3; j++ )
      if( t->m[k][j] < -65536 || t->m[k][j] > 65536 ) { c->setError( "vvr_set_output_transform: matrix entry beyond +-65536 (4.0 in Q14)" ); return VVR_ERR_PARAMETER; }
  if( !c->xform ) c->xform.reset( new vvr_output_transform );
  *c->xform = *t;
  c->xformStale = true;
  return VVR_OK;
}

VVR_API int vvr_set_output_lut3d( vvr_context* c, int n, const uint16_t* nodes )
{
  if( !c ) return VVR_ERR_PARAMETER;
  std::lock_guard<std::mutex> lk( c->mu );
  if( !nodes && n == 0 ) { c->lutN = 0; c->lut.clear(); return VVR_OK; }
  if( !nodes ) { c->setError( "vvr_set_output_lut3d: nodes is NULL with a size other than 0" ); return VVR_ERR_PARAMETER; }
  if( n != 17 && n != 33 && n != 65 ) { c->setError( "vvr_set_output_lut3d: the size is 17, 33 or 65 nodes per axis" ); return VVR_ERR_PARAMETER; }
  // the copy as the device takes it: a node is R, G, B, 0 - one 8-byte load per vertex
  const size_t count = (size_t) n * n * n;
  c->lut.assign( count * 4, 0 );
  for( size_t j = 0; j < count; j++ ) for( int k = 0; k < 3; k++ ) c->lut[4 * j + k] = nodes[3 * j + k];
  c->lutN = n; c->lutStale = true;
  return VVR_OK;
}

// the colour science of the presets, every formula as vvr.h gives it, in double
namespace {
struct PresetMath
{
  const double m1 = 2610. / 16384, m2 = 2523. / 4096 * 128, c1 = 3424. / 4096, c2 = 2413. / 4096 * 32, c3 = 2392. / 4096 * 32;
  const double ha = 0.17883277, hb = 1 - 4 * ha, hc = 0.5 - ha * std::log( 4 * ha );
  double lo = 0, hi = 1, maxLum = 1, ks = 1;
  PresetMath( double srcPeak, double dstPeak ) { lo = pqInv( 0 ); hi = pqInv( srcPeak ); maxLum = ( pqInv( dstPeak ) - lo ) / ( hi - lo ); ks = 1.5 * maxLum - 0.5; }
  static uint16_t q16( double v ) { return (uint16_t) std::floor( v * 65535 + 0.5 ); }
  double pqEotf( double e ) const { const double p = std::pow( e, 1 / m2 ); return 10000 * std::pow( std::max( p - c1, 0. ) / ( c2 - c3 * p ), 1 / m1 ); }
  double pqInv( double nits ) const { const double y = std::pow( nits / 10000, m1 ); return std::pow( ( c1 + c2 * y ) / ( 1 + c3 * y ), m2 ); }
  double eetf( double e ) const
  {
    const double e1 = std::min( std::max( ( e - lo ) / ( hi - lo ), 0. ), 1. );
    double e2 = e1;
    if( ks < 1 && e1 >= ks )
    {
      const double t = ( e1 - ks ) / ( 1 - ks ), t2 = t * t, t3 = t2 * t;
      e2 = ( 2 * t3 - 3 * t2 + 1 ) * ks + ( t3 - 2 * t2 + t ) * ( 1 - ks ) + ( -2 * t3 + 3 * t2 ) * maxLum;
    }
    return e2 * ( hi - lo ) + lo;
  }
  double hlgInv( double e ) const { return e <= 0.5 ? e * e / 3 : ( std::exp( ( e - hc ) / ha ) + hb ) / 12; }
  static double oetf( int target, double x )
  {
    return target == VVR_XFORM_TO_SRGB ? ( x <= 0.0031308 ? 12.92 * x : 1.055 * std::pow( x, 1 / 2.4 ) - 0.055 ) : target == VVR_XFORM_TO_BT709 ? ( x < 0.018 ? 4.5 * x : 1.099 * std::pow( x, 0.45 ) - 0.099 ) : x;
  }
  // the normalised primary matrix RGB -> XYZ of a gamut from its chromaticities (SMPTE RP 177), D65
  static void npm( int primaries, double n[3][3] )
  {
    const double xy709[3][2] = { { 0.640, 0.330 }, { 0.300, 0.600 }, { 0.150, 0.060 } }, xy2020[3][2] = { { 0.708, 0.292 }, { 0.170, 0.797 }, { 0.131, 0.046 } };
    const double ( *xy )[2] = primaries == 1 ? xy709 : xy2020;
    const double wx = 0.3127, wy = 0.3290, w[3] = { wx / wy, 1, ( 1 - wx - wy ) / wy };
    double p[3][3], inv[3][3];
    for( int j = 0; j < 3; j++ ) { p[0][j] = xy[j][0] / xy[j][1]; p[1][j] = 1; p[2][j] = ( 1 - xy[j][0] - xy[j][1] ) / xy[j][1]; }
    const double det = p[0][0] * ( p[1][1] * p[2][2] - p[1][2] * p[2][1] ) - p[0][1] * ( p[1][0] * p[2][2] - p[1][2] * p[2][0] ) + p[0][2] * ( p[1][0] * p[2][1] - p[1][1] * p[2][0] );
    for( int i = 0; i < 3; i++ ) for( int j = 0; j < 3; j++ )
      inv[j][i] = ( p[( i + 1 ) % 3][( j + 1 ) % 3] * p[( i + 2 ) % 3][( j + 2 ) % 3] - p[( i + 1 ) % 3][( j + 2 ) % 3] * p[( i + 2 ) % 3][( j + 1 ) % 3] ) / det;
    for( int j = 0; j < 3; j++ ) { const double sc = inv[j][0] * w[0] + inv[j][1] * w[1] + inv[j][2] * w[2]; for( int i = 0; i < 3; i++ ) n[i][j] = p[i][j] * sc; }
  }
  // M = inverse( N709 ) * Nsrc; source primaries 1: the identity
  static void gamut( int primaries, double M[3][3] )
  {
    for( int k = 0; k < 3; k++ ) for( int j = 0; j < 3; j++ ) M[k][j] = k == j;
    if( primaries == 1 ) return;
    double a[3][3], b[3][3], ai[3][3];
    npm( 1, a ); npm( primaries, b );
    const double det = a[0][0] * ( a[1][1] * a[2][2] - a[1][2] * a[2][1] ) - a[0][1] * ( a[1][0] * a[2][2] - a[1][2] * a[2][0] ) + a[0][2] * ( a[1][0] * a[2][1] - a[1][1] * a[2][0] );
    for( int i = 0; i < 3; i++ ) for( int j = 0; j < 3; j++ )
      ai[j][i] = ( a[( i + 1 ) % 3][( j + 1 ) % 3] * a[( i + 2 ) % 3][( j + 2 ) % 3] - a[( i + 1 ) % 3][( j + 2 ) % 3] * a[( i + 2 ) % 3][( j + 1 ) % 3] ) / det;
    for( int k = 0; k < 3; k++ ) for( int j = 0; j < 3; j++ ) M[k][j] = ai[k][0] * b[0][j] + ai[k][1] * b[1][j] + ai[k][2] * b[2][j];
  }
};
bool presetKnown( int transfer, int primaries, int target, double srcPeak, double dstPeak )
{
  if( ( transfer != 16 && transfer != 18 ) || ( primaries != 1 && primaries != 9 ) || target < VVR_XFORM_TO_SRGB || target > VVR_XFORM_TO_LINEAR ) return false;
  return transfer != 16 || ( srcPeak > 0 && srcPeak <= 10000 && dstPeak > 0 && dstPeak <= 10000 );
}
}   // namespace

VVR_API int vvr_output_transform_preset( vvr_output_transform* out, int transfer, int primaries, int target, double srcPeak, double dstPeak, int bitDepth )
{
  if( !out || !presetKnown( transfer, primaries, target, srcPeak, dstPeak ) || bitDepth < 8 || bitDepth > 10 ) return VVR_ERR_PARAMETER;
  const PresetMath pm( srcPeak, dstPeak );
  vvr_output_transform t; memset( &t, 0, sizeof( t ) );
  t.struct_size = sizeof( t );
  // stage 1: PQ EOTF behind the BT.2390 EETF, or the inverse HLG OETF
  const int top = ( 1 << bitDepth ) - 1;
  for( int v = 0; v <= top; v++ )
  {
    const double e = (double) v / top;
    t.lin[v] = pm.q16( transfer == 16 ? std::min( pm.pqEotf( pm.eetf( e ) ) / dstPeak, 1. ) : pm.hlgInv( e ) );
  }
  // stage 2: inverse( N709 ) * Nsrc, the normalised primary matrices from the chromaticities
  double M[3][3];
  pm.gamut( primaries, M );
  for( int k = 0; k < 3; k++ ) for( int j = 0; j < 3; j++ ) t.m[k][j] = (int32_t) std::floor( M[k][j] * 16384 + 0.5 );
  // stage 3: the target's OETF
  for( int i = 0; i <= 1024; i++ ) t.enc[i] = pm.q16( pm.oetf( target, std::min( 64 * i, 65535 ) / 65535. ) );
  *out = t;
  return VVR_OK;
}

// the 3-D LUT of the same cases with the tone curve on luminance: BT.2390's EETF on Y (PQ), the HLG OOTF with its system gamma (vvr.h)
VVR_API int vvr_output_lut3d_preset( uint16_t* nodes, int n, int transfer, int primaries, int target, double srcPeak, double dstPeak )
{
  if( !nodes || ( n != 17 && n != 33 && n != 65 ) || !presetKnown( transfer, primaries, target, srcPeak, dstPeak ) ) return VVR_ERR_PARAMETER;
  if( transfer == 18 && !( dstPeak > 0 && dstPeak <= 10000 ) ) return VVR_ERR_PARAMETER;      // (Lw of the system gamma)
  const PresetMath pm( srcPeak, dstPeak );
  double M[3][3], N[3][3];
  pm.gamut( primaries, M ); pm.npm( primaries, N );
  const double* w = N[1];      // (luminance of the source's R, G, B)
  const double gamma = dstPeak >= 400 && dstPeak <= 2000 ? 1.2 + 0.42 * std::log10( dstPeak / 1000 ) : 1.2 * std::pow( 1.111, std::log2( dstPeak / 1000 ) );
  const int S = 65536 / ( n - 1 );
  std::vector<double> lin( n );      // per node of an axis: display light in cd/m2 (PQ) or scene light 0 .. 1 (HLG)
  for( int j = 0; j < n; j++ ) { const double e = std::min( j * S, 65535 ) / 65535.; lin[j] = transfer == 16 ? pm.pqEotf( e ) : pm.hlgInv( e ); }
  for( int jb = 0; jb < n; jb++ )
    for( int jg = 0; jg < n; jg++ )
      for( int jr = 0; jr < n; jr++ )
      {
        double L[3] = { lin[jr], lin[jg], lin[jb] };
        const double Y = w[0] * L[0] + w[1] * L[1] + w[2] * L[2];
        double scale;
        if( transfer == 16 ) scale = ( Y > 0 ? pm.pqEotf( pm.eetf( pm.pqInv( Y ) ) ) / Y : 1. ) / dstPeak;
        else scale = Y > 0 ? std::pow( Y, gamma - 1 ) : 0.;
        uint16_t* o = nodes + 3 * ( ( (size_t) jb * n + jg ) * n + jr );
        for( int k = 0; k < 3; k++ )
        {
          const double t = M[k][0] * ( L[0] * scale ) + M[k][1] * ( L[1] * scale ) + M[k][2] * ( L[2] * scale );
          o[k] = pm.q16( pm.oetf( target, std::min( std::max( t, 0. ), 1. ) ) );
        }
      }
  return VVR_OK;
}

// light levels from the statistics of a frame (vvr_stats_submit), every formula as vvr.h gives it, in double
VVR_API int vvr_light_level( const vvr_frame_stats* st, int transfer, uint32_t percentileE4, struct vvr_light_level* out )
{
  if( !st || !out || st->struct_size != sizeof( vvr_frame_stats ) || st->mode != VVR_STATS_RGB || st->bit_depth < 8 || st->bit_depth > 10 || !st->samples ) return VVR_ERR_PARAMETER;
  if( percentileE4 < 1 || percentileE4 > 10000 || ( transfer != 0 && transfer != 16 ) ) return VVR_ERR_PARAMETER;
  const int M = ( 1 << st->bit_depth ) - 1;
  uint64_t total = 0;
  for( int v = 0; v < 1024; v++ ) total += st->hist_maxrgb[v];
  if( total != st->samples ) return VVR_ERR_PARAMETER;
  struct vvr_light_level r; memset( &r, 0, sizeof( r ) );
  r.struct_size = sizeof( r ); r.transfer = (uint32_t) transfer;
  uint64_t cum = 0; bool found = false;
  for( int v = 0; v < 1024; v++ )
  {
    if( st->hist_maxrgb[v] ) r.max_code = (uint32_t) v;
    cum += st->hist_maxrgb[v];
    if( !found && cum * 10000 >= (uint64_t) percentileE4 * st->samples ) { r.pct_code = (uint32_t) v; found = true; }
  }
  if( transfer == 16 )
  {
    const PresetMath pm( 10000, 10000 );
    auto nits = [&]( uint32_t code ) { return pm.pqEotf( (double) std::min<uint32_t>( code, M ) / M ); };
    r.max_nits = nits( r.max_code ); r.pct_nits = nits( r.pct_code );
    for( int k = 0; k < 3; k++ ) r.maxscl_nits[k] = nits( st->max_c[k] );
    double sum = 0;
    for( int v = 0; v <= M; v++ ) if( st->hist_maxrgb[v] ) sum += (double) st->hist_maxrgb[v] * nits( (uint32_t) v );
    r.avg_nits = sum / (double) st->samples;
  }
  *out = r;
  return VVR_OK;
}

// PSNR from the sums of a comparison (vvr_compare_submit), the formula as vvr.h gives it, in double
VVR_API int vvr_compare_psnr( const vvr_frame_compare* cmp, double peak, double psnr[4] )
{
  if( !cmp || !psnr || cmp->struct_size != sizeof( vvr_frame_compare ) || cmp->bit_depth < 8 || cmp->bit_depth > 10 || !cmp->samples[0] ) return VVR_ERR_PARAMETER;
  if( !( peak > 0 ) ) peak = (double) ( ( 1u << cmp->bit_depth ) - 1 );
  auto db = [&]( double samples, double sse ) { return sse == 0 ? HUGE_VAL : 10.0 * std::log10( peak * peak * samples / sse ); };
  const int nc = cmp->num_components == 1 ? 1 : 3;
  double samples = 0, sse = 0;
  for( int k = 0; k < 3; k++ )
  {
    psnr[k] = k < nc ? db( (double) cmp->samples[k], (double) cmp->sse[k] ) : 0.0;
    if( k < nc ) { samples += (double) cmp->samples[k]; sse += (double) cmp->sse[k]; }
  }
  psnr[3] = db( samples, sse );
  return VVR_OK;
}

// mean SSIM from the sums of an SSIM request (vvr_ssim_submit), the formula as vvr.h gives it, in double
VVR_API int vvr_compare_ssim( const vvr_frame_ssim* sm, double ssim[4] )
{
  if( !sm || !ssim || sm->struct_size != sizeof( vvr_frame_ssim ) || sm->bit_depth < 8 || sm->bit_depth > 10 || !sm->windows[0] ) return VVR_ERR_PARAMETER;
  auto mean = [&]( double sum, double windows ) { return windows == 0 ? 0.0 : sum / ( windows * 16777216.0 ); };
  const int nc = sm->num_components == 1 ? 1 : 3;
  double sum = 0, windows = 0;
  for( int k = 0; k < 3; k++ )
  {
    ssim[k] = k < nc ? mean( (double) sm->sum[k], (double) sm->windows[k] ) : 0.0;
    if( k < nc ) { sum += (double) sm->sum[k]; windows += (double) sm->windows[k]; }
  }
  ssim[3] = mean( sum, windows );
  return VVR_OK;
}

// MS-SSIM from the sums of an MS-SSIM request (vvr_msssim_submit), the formula as vvr.h gives it, in double
VVR_API int vvr_compare_msssim( const vvr_frame_msssim* ms, const double* weights, double msssim[4] )
{
  if( !ms || !msssim || ms->struct_size != sizeof( vvr_frame_msssim ) || ms->bit_depth < 8 || ms->bit_depth > 10 || ms->scales < 1 || ms->scales > VVR_MSSSIM_MAX_SCALES ) return VVR_ERR_PARAMETER;
  static const double wang[VVR_MSSSIM_MAX_SCALES] = { 0.0448, 0.2856, 0.3001, 0.2363, 0.1333 };
  const int scales = (int) ms->scales, nc = ms->num_components == 1 ? 1 : 3;
  double wt[VVR_MSSSIM_MAX_SCALES], total = 0;
  for( int k = 0; k < scales; k++ ) total += wang[k];
  for( int k = 0; k < scales; k++ )
  {
    if( !ms->windows[k][0] ) return VVR_ERR_PARAMETER;
    wt[k] = weights ? weights[k] : wang[k] / total;
    if( !std::isfinite( wt[k] ) || wt[k] < 0 ) return VVR_ERR_PARAMETER;
  }
  double out[4] = { 0, 0, 0, 0 };
  for( int c = 0; c < 4; c++ )
  {
    bool exists = c == 3 || c < nc;      // (a component that does not exist, or lacks windows at one of the levels: 0)
    for( int k = 0; k < scales && c < 3 && exists; k++ ) exists = ms->windows[k][c] != 0;
    if( !exists ) continue;
    double product = 1;
    for( int k = 0; k < scales; k++ )
    {
      double sum = 0, windows = 0;
      for( int q = ( c < 3 ? c : 0 ); q < ( c < 3 ? c + 1 : nc ); q++ ) { sum += (double) ( k < scales - 1 ? ms->sum_cs[k][q] : ms->sum_v[k][q] ); windows += (double) ms->windows[k][q]; }
      const double m = sum / ( windows * 16777216.0 );
      product *= pow( m > 0 ? m : 0.0, wt[k] );
    }
    out[c] = product;
  }
  memcpy( msssim, out, sizeof( out ) );
  return VVR_OK;
}

// the block size and the grid of blocks of an XPSNR request (vvr_xpsnr_submit), as vvr.h gives them
VVR_API int vvr_xpsnr_blocks( int w, int h, uint32_t block, uint32_t* resolvedBlock, uint32_t* blocksX, uint32_t* blocksY )
{
  if( !resolvedBlock || !blocksX || !blocksY || w < 8 || h < 8 || ( block & 3 ) ) return VVR_ERR_PARAMETER;
  const uint64_t B = block ? block : (uint64_t) std::max( 4, 4 * (int) ( 32.0 * sqrt( (double) w * (double) h / 8294400.0 ) + 0.5 ) );
  const uint64_t bx = ( (uint64_t) w + B - 1 ) / B, by = ( (uint64_t) h + B - 1 ) / B;
  if( bx * by > VVR_XPSNR_MAX_BLOCKS ) return VVR_ERR_PARAMETER;
  *resolvedBlock = (uint32_t) B; *blocksX = (uint32_t) bx; *blocksY = (uint32_t) by;
  return VVR_OK;
}

// the taps of one output sample of an axis under vvr_set_output_resampling, as vvr.h defines them (what the tables of k_output_resample hold)
VVR_API int vvr_resample_taps( int filter, int n, int m, int phase, int i, int32_t* first, int16_t* weights )
{
  if( !first || !weights || filter < VVR_RESAMPLE_AREA || filter > VVR_RESAMPLE_CUBIC || !resample_axis_ok( n, m ) || phase < 1 || phase > 2 || i < 0 || i >= m ) return VVR_ERR_PARAMETER;
  int f = 0;
  const int count = resample_taps_of( filter, n, m, phase, i, f, weights );
  if( count <= 0 ) return VVR_ERR_PARAMETER;
  *first = f;
  return count;
}

// XPSNR from the records of an XPSNR request (vvr_xpsnr_submit), the formula as vvr.h gives it, in double, the blocks in ascending order
VVR_API int vvr_compare_xpsnr( const vvr_frame_xpsnr* f, const vvr_xpsnr_block* blocks, double aPic, double peak, double xpsnr[4] )
{
  if( !f || !blocks || !xpsnr || f->struct_size != sizeof( vvr_frame_xpsnr ) || f->bit_depth < 8 || f->bit_depth > 10 || !f->samples[0] ||
      !( (uint64_t) f->blocks_x * f->blocks_y ) || f->filter < 1 || f->filter > 2 ) return VVR_ERR_PARAMETER;
  const int nc = f->num_components == 1 ? 1 : 3;
  if( peak <= 0 ) peak = (double) ( ( 1u << f->bit_depth ) - 1 );
  if( aPic <= 0 ) aPic = ldexp( 1.0, 2 * (int) f->bit_depth - 9 ) * sqrt( 3840.0 * 2160.0 / ( (double) f->width[0] * (double) f->height[0] ) );
  const double root = sqrt( aPic ), floorAct = ldexp( 1.0, (int) f->bit_depth - 6 );
  double wsse[3] = { 0, 0, 0 };
  for( uint64_t k = 0; k < (uint64_t) f->blocks_x * f->blocks_y; k++ )
  {
    const vvr_xpsnr_block& b = blocks[k];
    const double q = (double) b.count * ( f->filter == 2 ? 4 : 1 );
    double act = b.count ? 1 + (double) b.act_spatial / q + 2 * (double) b.act_temporal / q : 0;
    act = std::max( act, floorAct );
    const double wk = root / act;
    for( int c = 0; c < nc; c++ ) wsse[c] += wk * (double) b.sse[c];
  }
  double out[4] = { 0, 0, 0, 0 }, allW = 0, allN = 0;
  for( int c = 0; c < nc; c++ )
  {
    out[c] = wsse[c] == 0 ? HUGE_VAL : 10 * log10( peak * peak * (double) f->samples[c] / wsse[c] );
    allW += wsse[c]; allN += (double) f->samples[c];
  }
  out[3] = allW == 0 ? HUGE_VAL : 10 * log10( peak * peak * allN / allW );
  memcpy( xpsnr, out, sizeof( out ) );
  return VVR_OK;
}

VVR_API int vvr_read_output_grain( vvr_context* c, int slot, int x, int y, int w, int h, int bytesPerSample, void* const dst[3], const size_t dstStrideBytes[3] )
{
  if( !c || slot < 0 || slot >= (int) c->slots.size() || !c->slots[slot].p[0] || !dst || !dstStrideBytes ) return VVR_ERR_PARAMETER;
  if( !c->grainBank ) { c->setError( "vvr_read_output_grain: no film grain bank set" ); return VVR_ERR_PARAMETER; }
  const int bd = c->cfg.bit_depth, nc = c->cfg.chroma_format ? 3 : 1;
  if( bd != 8 && bd != 10 ) { c->setError( "vvr_read_output_grain: film grain needs a bit depth of 8 or 10 (FilmGrainImpl::set_depth)" ); return VVR_ERR_PARAMETER; }
  const DevPlanes d = pictureIn( c, slot );
  if( x < 0 || y < 0 || w <= 0 || h <= 0 || x + w > d.w[0] || y + h > d.h[0] || ( nc > 1 && ( ( x | y | w | h ) & 1 ) ) )
  { c->setError( "vvr_read_output_grain: window outside the picture, or odd in 4:2:0" ); return VVR_ERR_PARAMETER; }
  if( w <= 128 ) { c->setError( "vvr_read_output_grain: film grain needs a frame wider than 128 samples (FilmGrainImpl::add_grain_block)" ); return VVR_ERR_PARAMETER; }
  if( bytesPerSample != 1 && bytesPerSample != 2 ) { c->setError( "vvr_read_output_grain: bad sample size" ); return VVR_ERR_PARAMETER; }
  if( bytesPerSample == 1 && bd > 8 ) { c->setError( "vvr_read_output_grain: 8-bit output of a stream with more than 8 bits per sample (only narrowing of 8-bit content, vvdecimpl.cpp:853)" ); return VVR_ERR_PARAMETER; }
  for( int k = 0; k < nc; k++ )
    if( !dst[k] || dstStrideBytes[k] < (size_t) ( w >> ( k ? 1 : 0 ) ) * bytesPerSample ) { c->setError( "vvr_read_output_grain: missing plane or stride below the window's row" ); return VVR_ERR_PARAMETER; }
  hipSetDevice( c->device );
  int rc = vvr_sync( c ); if( rc != VVR_OK ) return rc;
  // the scratch: the packed planes, then the blocks' random words (staged in the pinned half at the same offset)
  FilmGrainParams p;
  size_t total = 0;
  for( int k = 0; k < 3; k++ )
  {
    const int s = k ? 1 : 0;
    p.src[k] = k < nc ? d.p[k] + (size_t) ( y >> s ) * d.stride[k] + ( x >> s ) : nullptr;
    p.stride[k] = d.stride[k]; p.w[k] = w >> s; p.h[k] = h >> s; p.dstOff[k] = total;
    if( k < nc ) total = alignUp( total + (size_t) p.w[k] * p.h[k] * bytesPerSample, 256 );
  }
  const int nbx = ( w + 15 ) / 16, nby = ( h + 15 ) / 16;
  const size_t wordsBytes = (size_t) nbx * nby * sizeof( uint32_t );
  if( ( rc = ensureOutputScratch( c, total + wordsBytes, total + wordsBytes ) ) != VVR_OK ) return rc;
  uint32_t* words = (uint32_t*) ( (char*) c->outHost + total );
  const uint32_t nextSeed = grain_words( c->grainSeed, nbx, nby, words );
  hipStream_t s = c->streams[0];
  if( !c->grainBankDev ) HIPCHK( c, hipMalloc( &c->grainBankDev, sizeof( vvr_film_grain_bank ) ) );
  if( c->grainBankStale ) HIPCHK( c, hipMemcpyAsync( c->grainBankDev, c->grainBank.get(), sizeof( vvr_film_grain_bank ), hipMemcpyHostToDevice, s ) );
  HIPCHK( c, hipMemcpyAsync( (char*) c->outDev + total, words, wordsBytes, hipMemcpyHostToDevice, s ) );
  p.bank = (const vvr_film_grain_bank*) c->grainBankDev; p.words = (const uint32_t*) ( (char*) c->outDev + total ); p.nbx = nbx;
  p.numComp = nc; p.bs = bd - 8; p.scaleShift = c->grainBank->shift + 6 - p.bs; p.bytesPerSample = bytesPerSample;
  launch_film_grain( s, p, c->outDev );
  HIPCHK( c, hipGetLastError() );
  HIPCHK( c, hipMemcpyAsync( c->outHost, c->outDev, total, hipMemcpyDeviceToHost, s ) );
  HIPCHK( c, hipStreamSynchronize( s ) );
  c->grainBankStale = false;
  c->grainSeed = nextSeed;      // (only a frame that was grained advances the chain)
  for( int k = 0; k < nc; k++ )
  {
    const size_t rowBytes = (size_t) p.w[k] * bytesPerSample;
    for( int r = 0; r < p.h[k]; r++ ) memcpy( (uint8_t*) dst[k] + (size_t) r * dstStrideBytes[k], (const uint8_t*) c->outHost + p.dstOff[k] + (size_t) r * rowBytes, rowBytes );
  }
  return VVR_OK;
}

VVR_API int vvr_read_picture( vvr_context* c, int slot, uint16_t* const* dst, const size_t* dstStrideSamples, int threads )
{
  if( !c || slot < 0 || slot >= (int) c->slots.size() || !dst || !dstStrideSamples ) return VVR_ERR_PARAMETER;
  hipSetDevice( c->device );
  const DevPlanes d = pictureIn( c, slot );
  const int nc = c->cfg.chroma_format ? 3 : 1;
  // (several threads may be in here at once: the error text is set under the context's lock)
  for( int k = 0; k < nc; k++ ) if( !dst[k] || dstStrideSamples[k] < (size_t) d.w[k] ) { std::lock_guard<std::mutex> lk( c->mu ); c->setError( "vvr_read_picture: missing plane or stride below the picture's width" ); return VVR_ERR_PARAMETER; }
  // pinned staging of one picture; concurrent callers (the pictures a decoder finishes side by side) take one each
  void* host = nullptr;
  {
    std::lock_guard<std::mutex> lk( c->mu );
    if( !c->outStream ) HIPCHK( c, hipStreamCreateWithFlags( &c->outStream, hipStreamNonBlocking ) );
    if( !c->stagePool.empty() ) { host = c->stagePool.back(); c->stagePool.pop_back(); }
  }
  if( !host && hipHostMalloc( &host, c->slotBytes, hipHostMallocDefault ) != hipSuccess ) { std::lock_guard<std::mutex> lk( c->mu ); c->setError( "vvr_read_picture: out of pinned memory" ); return VVR_ERR_DEVICE; }
  size_t off[3] = { 0, 0, 0 }, total = 0;
  for( int k = 0; k < nc; k++ ) { off[k] = total; total += alignUp( (size_t) d.w[k] * d.h[k] * sizeof( pel_t ), 256 ); }
  hipError_t e = hipSuccess;
  for( int k = 0; k < nc && e == hipSuccess; k++ )
    e = hipMemcpy2DAsync( (char*) host + off[k], (size_t) d.w[k] * sizeof( pel_t ), d.p[k], (size_t) d.stride[k] * sizeof( pel_t ), (size_t) d.w[k] * sizeof( pel_t ), d.h[k], hipMemcpyDeviceToHost, c->outStream );
  hipEvent_t done = nullptr;
  if( e == hipSuccess ) e = hipEventCreateWithFlags( &done, hipEventDisableTiming );
  if( e == hipSuccess ) e = hipEventRecord( done, c->outStream );
  if( e == hipSuccess ) e = hipEventSynchronize( done );
  if( done ) hipEventDestroy( done );
  if( e == hipSuccess )
  {
    // rows out of the staging buffer at the caller's strides, on `threads` threads (one plane after the other would leave the copy to one core's bandwidth)
    int rows = 0; for( int k = 0; k < nc; k++ ) rows += d.h[k];
    const int nt = std::max( 1, std::min( threads, 16 ) );
    auto part = [&]( int t )
    {
      int r0 = (int) ( (int64_t) rows * t / nt ), r1 = (int) ( (int64_t) rows * ( t + 1 ) / nt ), base = 0;
      for( int k = 0; k < nc; k++ )
      {
        for( int r = std::max( r0, base ); r < std::min( r1, base + d.h[k] ); r++ )
          memcpy( dst[k] + (size_t) ( r - base ) * dstStrideSamples[k], (const char*) host + off[k] + (size_t) ( r - base ) * d.w[k] * sizeof( pel_t ), (size_t) d.w[k] * sizeof( pel_t ) );
        base += d.h[k];
      }
    };
    if( nt == 1 ) part( 0 );
    else { std::vector<std::thread> th; for( int t = 1; t < nt; t++ ) th.emplace_back( part, t ); part( 0 ); for( auto& t : th ) t.join(); }
  }
  {
    std::lock_guard<std::mutex> lk( c->mu );
    c->stagePool.push_back( host );
    if( e != hipSuccess ) { c->setError( std::string( "vvr_read_picture: " ) + hipGetErrorString( e ) ); return VVR_ERR_DEVICE; }
  }
  return VVR_OK;
}

VVR_API int vvr_picture_hash( vvr_context* c, int slot, int method, uint8_t* digest, int* digestLen )
{
  if( !c || slot < 0 || slot >= (int) c->slots.size() || !digest || method < VVR_HASH_MD5 || method > VVR_HASH_CHECKSUM ) return VVR_ERR_PARAMETER;
  hipSetDevice( c->device );
  int rc = vvr_sync( c ); if( rc != VVR_OK ) return rc;
  const DevPlanes d = pictureIn( c, slot );      // (the picture in the slot, not the slot)
  const int nc = c->cfg.chroma_format ? 3 : 1, len = method == VVR_HASH_MD5 ? 16 : method == VVR_HASH_CRC ? 2 : 4;
  const bool two = c->cfg.bit_depth > 8;
  hipStream_t s = c->streams[0];
  if( method == VVR_HASH_MD5 )
  {
    // MD5 over the sample bytes in raster order (calcMD5, PicYuvMD5.cpp:197): the plane is packed on the device to exactly those bytes, copied, hashed here
    for( int k = 0; k < nc; k++ )
    {
      const size_t bytes = (size_t) d.w[k] * d.h[k] * ( two ? 2 : 1 );
      if( ( rc = ensureOutputScratch( c, alignUp( bytes, 256 ), alignUp( bytes, 256 ) ) ) != VVR_OK ) return rc;
      launch_output_window( s, d.p[k], d.stride[k], d.w[k], d.h[k], two ? 2 : 1, c->outDev );
      HIPCHK( c, hipMemcpyAsync( c->outHost, c->outDev, bytes, hipMemcpyDeviceToHost, s ) );
      HIPCHK( c, hipStreamSynchronize( s ) );
      Md5 m; m.update( (const uint8_t*) c->outHost, bytes ); m.finish( digest + (size_t) k * len );
    }
  }
  else
  {
    // CRC (compCRC, :99-137) and checksum (compChecksum, :152-176): per-row partial results from the device, combined here
    size_t rowsTotal = 0; for( int k = 0; k < nc; k++ ) rowsTotal += d.h[k];
    const size_t bytes = alignUp( sizeof( uint32_t ) * rowsTotal, 256 );
    if( ( rc = ensureOutputScratch( c, bytes, bytes ) ) != VVR_OK ) return rc;
    uint32_t* dev = (uint32_t*) c->outDev; const uint32_t* host = (const uint32_t*) c->outHost;
    size_t off = 0;
    bool timed = false; PendingTiming t; double planesBytes = 0;
    for( int k = 0; k < nc; k++ ) planesBytes += (double) d.w[k] * d.h[k] * sizeof( pel_t );
    outTimeBegin( c, s, timed, t, K_PLANE_HASH_ROWS, planesBytes + sizeof( uint32_t ) * rowsTotal );      // (one entry for the planes' launches together)
    for( int k = 0; k < nc; k++ ) { launch_plane_hash_rows( s, d.p[k], d.stride[k], d.w[k], d.h[k], two ? 1 : 0, method == VVR_HASH_CRC ? 1 : 0, dev + off ); off += d.h[k]; }
    if( timed ) hipEventRecord( t.b, s );
    hipError_t he = hipGetLastError();
    if( he == hipSuccess ) he = hipMemcpyAsync( c->outHost, c->outDev, sizeof( uint32_t ) * rowsTotal, hipMemcpyDeviceToHost, s );
    if( he == hipSuccess ) he = hipStreamSynchronize( s );
    if( he != hipSuccess )
    {
      if( timed ) { hipEventDestroy( t.a ); hipEventDestroy( t.b ); }      // (nothing is counted for a call that failed)
      c->setError( std::string( "vvr_picture_hash: " ) + hipGetErrorString( he ) );
      return VVR_ERR_DEVICE;
    }
    { std::lock_guard<std::mutex> lk( c->mu ); outTimeEnd( c, timed, t, nc ); }
    off = 0;
    for( int k = 0; k < nc; k++ )
    {
      uint8_t* out = digest + (size_t) k * len;
      if( method == VVR_HASH_CRC )
      {
        const uint32_t xRow = crcXPow( (uint64_t) d.w[k] * ( two ? 16 : 8 ) );
        uint32_t crc = 0xffff;
        for( int r = 0; r < d.h[k]; r++ ) crc = crcMul( crc, xRow ) ^ ( host[off + r] & 0xffff );
        crc = crcMul( crc, crcXPow( 16 ) );                  // the 16 zero bits appended at the end
        out[0] = (uint8_t) ( crc >> 8 ); out[1] = (uint8_t) crc;
      }
      else
      {
        uint32_t sum = 0;
        for( int r = 0; r < d.h[k]; r++ ) sum += host[off + r];
        out[0] = (uint8_t) ( sum >> 24 ); out[1] = (uint8_t) ( sum >> 16 ); out[2] = (uint8_t) ( sum >> 8 ); out[3] = (uint8_t) sum;
      }
      off += d.h[k];
    }
  }
  if( digestLen ) *digestLen = len;
  return VVR_OK;
}

}   // extern "C"

// =====================================================================================================================
// output queue: the output stage as a pipeline.  A request is ordered behind its picture's `done` event on the context's output stream,
// runs there (k_film_grain, k_rescale - or, under vvr_set_output_resampling, k_output_resample in its place -, k_output_frame, k_output_narrow, k_output_rgb or k_output_yuv as the request needs them), leaves through a ring entry (device scratch + pinned
// staging) and is collected with its ticket.  Nothing here calls vvr_sync.  The slot is protected the way an external reader's is
// (vvr_slot_external_event): the entry's `read` event, recorded behind the last kernel of the request, is registered with the slot, so a
// picture submitted afterwards that overwrites the slot waits for it on the device - not for the copy to the host.
// k_rescale and k_film_grain reach the packed format and the chained case with at most one extra pass through HBM: they store 16-bit samples
// into the entry's scratch (`tmp`) and k_output_frame packs (or interleaves: NV12, P010) from there, or k_output_rgb converts from there (the RGB
// formats; a plain request converts straight from the slot); into the planar formats they store directly as ever - but for VVR_OUT_PLANAR8 of a
// context of 9 or 10 bits (vvr_set_output_narrowing), which goes through 16-bit samples and k_output_narrow like VVR_OUT_NV12.
// A request whose destination planes lie in device memory the context knows (vvr_device_alloc / vvr_device_register) moves nothing over PCIe:
// k_output_frame stores a plane whose rows are back to back at a 32-byte aligned base straight into it, exactly its bytes; every other plane
// (padded rows, odd bases, the planes k_film_grain / k_rescale store themselves) goes through the entry's scratch and one device-to-device
// hipMemcpy2DAsync at the caller's stride.  `done` is recorded behind the last kernel or copy; vvr_output_stream_wait hands it to a stream.
// A hash request (vvr_hash_submit) is an entry with no destination planes: k_hash_rows and k_hash_combine leave one word per component in the
// entry's scratch and that is all that crosses PCIe (CRC, checksum), or k_output_window packs the planes and their bytes cross (MD5: hashed by
// the thread that calls vvr_output_wait); the digest bytes and the comparison with the SEI's are made in vvr_output_wait.
// A statistics request (vvr_stats_submit) is an entry with no destination planes either: its scratch holds the copies of the words the workgroups
// add into - cleared on the output stream ahead of the launch - and the words k_output_stats_sum folds them to, which are all that crosses PCIe;
// vvr_output_wait writes the caller's vvr_frame_stats from them.
// A comparison request (vvr_compare_submit) reads two sources: the slot and a second slot, the caller's device memory in place, or the entry's
// `tmp`, where a reference from the host is packed (copied from the caller's pinned memory, or through the entry's pinned staging).  Its scratch
// holds a record per block and component, every word of which k_output_compare stores - nothing is cleared - then the words
// k_output_compare_sum folds them to and the map; the words (with `map` the map too) are all that crosses PCIe back.
// An SSIM request (vvr_ssim_submit) is a comparison request with other kernels (k_output_ssim, k_output_ssim_sum), records and words: both calls
// go through compareSubmit.  So does an MS-SSIM request (vvr_msssim_submit): a k_output_msssim per scale, each but the last writing the next
// level of both images into the pyramid that lies behind the records and words in the entry's `dev`, and one k_output_msssim_sum; only level 0
// reads the slots and the reference, so `read` is recorded behind it.  And an XPSNR request (vvr_xpsnr_submit): its prev planes take the
// reference's steps - home, staging behind the reference's planes, devRanges bookkeeping - its records are cleared on the stream and added to
// by one k_output_xpsnr, and they cross PCIe as they are: vvr_output_wait sums them.
// Under vvr_set_compare_scaling the four measures take a reference of another size: the window is validated as it is, everything behind it is
// sized by the size that is set.  An SSIM, MS-SSIM or XPSNR request runs k_rescale per component into 16-bit planes at the end of its `dev`
// and measures those (the `read` event sits behind the last k_rescale); a comparison request is one k_output_compare_scaled, which rescales and
// compares in one pass into records its launcher has cleared.
// =====================================================================================================================
#define VVR_OUT_RING 8
enum { OQ_FREE = 0, OQ_FLIGHT, OQ_WAITING };
struct OutEntry {
  int state = OQ_FREE, ticket = -1, job = -1, slot = -1, rc = VVR_OK;
  char* dev = nullptr;  size_t devCap = 0;       // the output as it crosses PCIe: planes at off[], rows back to back
  char* tmp = nullptr;  size_t tmpCap = 0;       // 16-bit intermediate planes (grained, rescaled) and the grain's random words
  char* host = nullptr; size_t hostCap = 0;      // pinned: the output (unless it goes straight to the caller's pinned memory), then the words
  hipEvent_t read = nullptr, done = nullptr;     // behind the last kernel; behind the last copy
  bool direct = false, queued = false;           // direct: vvr_output_wait copies nothing (pinned or device destinations); queued: something was enqueued (done has been recorded)
  bool devDst = false; size_t extent[5] = { 0, 0, 0, 0, 0 };      // the destination planes lie in device memory: dst[k] .. dst[k] + extent[k] (five: an XPSNR request's reference and prev planes)
  int nc = 0, rows[3] = { 0, 0, 0 }; size_t off[3] = { 0, 0, 0 }, rowBytes[3] = { 0, 0, 0 }, dstStride[3] = { 0, 0, 0 }; void* dst[5] = { nullptr, nullptr, nullptr, nullptr, nullptr };
  // a batch (vvr_output_submit_batch; a single request: one region): plane k of region i at off[k] + i * step[k] in `dev` / `host` and at dst[k] + i * bstride[k]
  int count = 1; size_t step[3] = { 0, 0, 0 }, bstride[3] = { 0, 0, 0 };
  bool timed = false; PendingTiming timing;
  // a hash request: method + 1 (0: an output request); planes of planeBytes[] at off[] in `host` (MD5) or one word per component at its start
  int hash = 0, hashNc = 0; size_t planeBytes[3] = { 0, 0, 0 };
  uint8_t* digest = nullptr; uint32_t* mismatch = nullptr; bool verify = false; uint8_t expected[48];
  bool timed2 = false; PendingTiming timing2;      // (k_hash_combine; `timing` is k_hash_rows then)
  bool timed0 = false; PendingTiming timing0; int rescales = 0;      // (the k_rescale launches ahead of a measure under vvr_set_compare_scaling, or the k_output_resample launches of an output request under vvr_set_output_resampling, and how many)
  // a statistics request: mode + 1 (0: none); STATS_WORDS words at the start of `host`; what vvr_output_wait writes besides them
  int stats = 0, statsW = 0, statsH = 0; vvr_frame_stats* statsOut = nullptr;
  // a comparison request: its number of components (0: none); CMP_OUT_WORDS words per component at the start of `host`, the map's words from
  // word CMP_HEAD_WORDS on; the second slot it reads (-1: none); what vvr_output_wait writes
  int cmp = 0, cmpW = 0, cmpH = 0, cmpBlocks = 0, refSlot = -1; vvr_frame_compare* cmpOut = nullptr; uint32_t* cmpMap = nullptr;
  // ... or an SSIM request, which is a comparison request with records and words of its own (SSIM_OUT_WORDS per component) and with cmpOut and
  // cmpMap pointing to a vvr_frame_ssim and to int32_t words
  bool cmpSsim = false;
  // ... or an MS-SSIM request (msScales > 0: its number of scales), a comparison request too: MSSSIM_OUT_WORDS words per level and component at the
  // start of `host`, cmpOut pointing to a vvr_frame_msssim, no map; `dev` holds the records of all levels, the words, then the pyramid
  int msScales = 0;
  // ... or an XPSNR request (xps), a comparison request too: its records - blocks of XPSNR_REC_WORDS 64-bit words, a vvr_xpsnr_block each - at the
  // start of `dev` (cleared, then added to by k_output_xpsnr) and of `host`; cmpOut points to a vvr_frame_xpsnr; what vvr_output_wait writes
  bool xps = false; int xpsTemporal = 0, xpsFilter = 0, xpsBlock = 0, xpsBx = 0, xpsBy = 0; vvr_xpsnr_block* xpsBlocks = nullptr;
};
// what vvr_xpsnr_submit adds to a comparison request: checked values (temporal 0 .. 2, filter resolved or 0, block 0 or a multiple of 4) and the prev planes
struct XpsnrAsk { int temporal, filter; uint32_t block; const void* prev[2]; size_t prevStride[2]; vvr_xpsnr_block* blocks; };
#define CMP_HEAD_WORDS 32      /* 3 x CMP_OUT_WORDS, rounded up: the map starts at a multiple of 128 bytes */

// The tap tables of k_output_resample (vvr_set_output_resampling): built on the host from the integer definition (resample_taps_of), one per
// ( n, m, phi, filter ), laid out as ResampleParams takes them (vvr_device.h), and kept in device memory - eight of them, the least recently
// used one replaced.  A request needs at most four (luma and chroma, two axes), so a stream of requests of one geometry uploads nothing.  Every
// table has device and pinned memory of a fixed size of its own, allocated on first use and kept until vvr_destroy: nothing in the request
// path frees device memory.  A table is uploaded on the output stream, behind the kernels of the requests in flight that read the one it
// replaces; `uploaded` is recorded behind the copy, and the pinned image is rewritten only once that has completed.
// Size: count <= 4 n / m + 2, so the weights of an axis are at most 4 n + 2 m <= 49 152 words of 16 bits, behind m <= 8192 words of 32 bits.
#define VVR_RESAMPLE_TABLES 8
#define VVR_RESAMPLE_TABLE_BYTES ( 192 << 10 )
struct ResampleTable {
  int n = 0, m = 0, phi = 0, filter = 0, taps = 0; uint64_t used = 0;
  char* dev = nullptr; char* host = nullptr; hipEvent_t uploaded = nullptr;
};

static void destroyOutputQueue( vvr_context* c )
{
  if( c->resampleTabs )
    for( int i = 0; i < VVR_RESAMPLE_TABLES; i++ )
    {
      ResampleTable& t = c->resampleTabs[i];
      if( t.dev ) hipFree( t.dev ); if( t.host ) hipHostFree( t.host ); if( t.uploaded ) hipEventDestroy( t.uploaded );
    }
  delete[] c->resampleTabs; c->resampleTabs = nullptr;
  if( c->outRing )
    for( int i = 0; i < VVR_OUT_RING; i++ )
    {
      OutEntry& e = c->outRing[i];
      if( e.dev ) hipFree( e.dev ); if( e.tmp ) hipFree( e.tmp ); if( e.host ) hipHostFree( e.host );
      if( e.read ) hipEventDestroy( e.read ); if( e.done ) hipEventDestroy( e.done );
      if( e.timed ) { hipEventDestroy( e.timing.a ); hipEventDestroy( e.timing.b ); }
      if( e.timed2 ) { hipEventDestroy( e.timing2.a ); hipEventDestroy( e.timing2.b ); }
      if( e.timed0 ) { hipEventDestroy( e.timing0.a ); hipEventDestroy( e.timing0.b ); }
    }
  delete[] c->outRing; c->outRing = nullptr;
  if( c->outQStream ) { hipStreamDestroy( c->outQStream ); c->outQStream = nullptr; }
}

namespace {
int outRefuse( vvr_context* c, const char* why, const char* who = "vvr_output_submit" ) { std::lock_guard<std::mutex> lk( c->mu ); c->setError( std::string( who ) + ": " + why ); return VVR_ERR_PARAMETER; }
size_t outRegion( size_t bytes ) { return alignUp( bytes + 32, 256 ); }      // (k_output_frame stores whole pieces: up to 31 bytes behind a plane)
int outGrow( char*& p, size_t& cap, size_t need, bool pinned )
{
  if( need <= cap ) return VVR_OK;
  if( p ) { if( pinned ) hipHostFree( p ); else hipFree( p ); }
  p = nullptr; cap = 0;
  const size_t want = alignUp( need, 1 << 16 );
  if( ( pinned ? hipHostMalloc( (void**) &p, want, hipHostMallocDefault ) : hipMalloc( (void**) &p, want ) ) != hipSuccess ) { p = nullptr; return VVR_ERR_DEVICE; }
  cap = want;
  return VVR_OK;
}
OutEntry* outFind( vvr_context* c, int ticket ) { if( c->outRing && ticket >= 0 ) for( int i = 0; i < VVR_OUT_RING; i++ ) if( c->outRing[i].state != OQ_FREE && c->outRing[i].ticket == ticket ) return &c->outRing[i]; return nullptr; }
// the request's picture failed (an error that only showed when the picture completed: the intra stage's bounded waits)?  done: the request's own work
// has finished, so the picture's has.  mu held (released while the picture's host event is waited for when `wait`).
int outJobStatus( vvr_context* c, int job, std::unique_lock<std::mutex>& lk, bool wait )
{
  if( job < 0 ) return VVR_OK;
  auto it = c->jobs.find( job );
  if( it == c->jobs.end() ) return VVR_OK;
  if( !it->second->completed && it->second->state == J_COMMITTED && it->second->doneHost )
  {
    hipEvent_t ev = it->second->doneHost;
    if( wait ) { lk.unlock(); hipEventSynchronize( ev ); lk.lock(); }
    else if( hipEventQuery( ev ) != hipSuccess ) return VVR_NOT_READY;
    it = c->jobs.find( job );
    if( it == c->jobs.end() ) return VVR_OK;
    if( !it->second->completed ) completeLocked( c, *it->second );
  }
  if( it->second->state == J_FAILED ) { c->setError( it->second->err ); return it->second->rc; }
  return VVR_OK;
}
// A request's way into the ring, shared by the four submit calls (`who`); mu held in all three helpers.
// outAcquire: a free entry, the output stream, the entry's events; the picture `job` reconstructs into `slot` has been handed to the device - the
// only host wait of a submit call, only when `blocking`, mu released meanwhile.  VVR_OK: jobDone is the event the request waits for on the device
// (NULL: the picture has finished), jobFailed the status of a picture that failed; anything else is what the submit call returns.
int outAcquire( vvr_context* c, const char* who, int slot, int job, bool blocking, std::unique_lock<std::mutex>& lk, OutEntry*& e, hipEvent_t& jobDone, int& jobFailed, OutEntry* take = nullptr )
{
  const std::string w = std::string( who ) + ": ";
  e = take; jobDone = nullptr; jobFailed = VVR_OK;      // (take: a free entry the caller has chosen - vvr_compare_submit, which has staged a reference in its pinned memory)
  if( !c->outRing ) c->outRing = new OutEntry[VVR_OUT_RING];
  for( int i = 0; i < VVR_OUT_RING && !e; i++ ) if( c->outRing[i].state == OQ_FREE ) e = &c->outRing[i];
  if( !e ) { c->setError( w + "8 requests in flight (vvr_output_wait retires one)" ); return VVR_ERR_BUSY; }
  if( !c->outQStream ) HIPCHK( c, hipStreamCreateWithFlags( &c->outQStream, hipStreamNonBlocking ) );
  if( !e->read ) HIPCHK( c, hipEventCreateWithFlags( &e->read, hipEventDisableTiming ) );
  if( !e->done ) HIPCHK( c, hipEventCreateWithFlags( &e->done, hipEventDisableTiming ) );
  if( job >= 0 )
  {
    auto it = c->jobs.find( job );
    if( it != c->jobs.end() )        // (else retired: finished long ago)
    {
      {
        const Job& j = *it->second;
        const vvr_pic_header* hd = j.q ? &j.q->hdr : ( j.pic.hdr.abi_version ? &j.pic.hdr : nullptr );
        if( hd && hd->out_slot != slot ) { c->setError( w + "the job does not reconstruct into this slot (hdr.out_slot)" ); return VVR_ERR_PARAMETER; }
      }
      if( !( it->second->state == J_COMMITTED || it->second->completed ) )
      {
        if( !blocking ) return VVR_NOT_READY;
        c->cv.wait( lk, [&]{ auto q = c->jobs.find( job ); return q == c->jobs.end() || q->second->state == J_COMMITTED || q->second->completed; } );
        it = c->jobs.find( job );
      }
      if( it != c->jobs.end() )
      {
        if( it->second->state == J_FAILED ) jobFailed = it->second->rc;
        else
        {
          // (the slot's writer is the first of its users: another one means that a later picture into the slot has been handed to the device already)
          if( !c->slotUsers[slot].empty() && c->slotUsers[slot][0] != job ) { c->setError( w + "a later picture that overwrites the slot has been submitted already (request a picture's output before the slot's next picture is submitted)" ); return VVR_ERR_PARAMETER; }
          if( !it->second->completed ) jobDone = it->second->done;
        }
      }
    }
  }
  else if( !c->bySeq.empty() )       // pictures still with the workers: who uses the slot is only known once they are committed
  {
    if( !blocking ) return VVR_NOT_READY;
    c->cv.wait( lk, [&]{ return c->bySeq.empty(); } );
  }
  if( e->state != OQ_FREE ) { c->setError( w + "called from two threads at once" ); return VVR_ERR_PARAMETER; }
  return VVR_OK;
}
// outTake: the entry gets its ticket (the caller sets OQ_FLIGHT when the request is accepted)
void outTake( vvr_context* c, OutEntry* e, int slot, int job, int jobFailed )
{
  e->ticket = c->nextTicket; c->nextTicket = c->nextTicket == 0x3fffffff ? 2 : c->nextTicket + 1;
  e->job = job; e->slot = slot; e->rc = jobFailed; e->queued = false; e->direct = false; e->devDst = false; e->nc = 0; e->count = 1; e->hash = 0; e->stats = 0; e->cmp = 0; e->msScales = 0; e->xps = false; e->refSlot = -1;
  if( e->timed ) { hipEventDestroy( e->timing.a ); hipEventDestroy( e->timing.b ); e->timed = false; }
  if( e->timed2 ) { hipEventDestroy( e->timing2.a ); hipEventDestroy( e->timing2.b ); e->timed2 = false; }
  if( e->timed0 ) { hipEventDestroy( e->timing0.a ); hipEventDestroy( e->timing0.b ); e->timed0 = false; }
  e->rescales = 0;
}
// outOrder: the output stream behind the picture (or, job < 0, behind the slot's users) and behind the external writers of the slot (readers cost nothing)
hipError_t outOrder( vvr_context* c, const OutEntry* e, int slot, int job, hipEvent_t jobDone )
{
  hipError_t rc = jobDone ? hipStreamWaitEvent( c->outQStream, jobDone, 0 ) : hipSuccess;
  if( job < 0 )
    for( int id : c->slotUsers[slot] )
    {
      auto it = c->jobs.find( id );
      if( rc == hipSuccess && it != c->jobs.end() && !it->second->completed && it->second->state == J_COMMITTED && it->second->done ) rc = hipStreamWaitEvent( c->outQStream, it->second->done, 0 );
    }
  for( hipEvent_t ev : c->slotExt[slot] ) if( rc == hipSuccess && ev != e->read ) rc = hipStreamWaitEvent( c->outQStream, ev, 0 );
  return rc;
}
// the tap table of an axis in device memory, uploaded on s if the context does not hold it; mu held
hipError_t resampleTable( vvr_context* c, hipStream_t s, int filter, int n, int m, int phi, const uint32_t*& tab, int& taps )
{
  if( !c->resampleTabs ) c->resampleTabs = new ResampleTable[VVR_RESAMPLE_TABLES];
  ResampleTable* t = nullptr;
  for( int i = 0; i < VVR_RESAMPLE_TABLES; i++ )
  {
    ResampleTable& q = c->resampleTabs[i];
    if( q.n == n && q.m == m && q.phi == phi && q.filter == filter ) { q.used = ++c->resampleUses; tab = (const uint32_t*) q.dev; taps = q.taps; return hipSuccess; }
    if( !t || q.used < t->used ) t = &q;
  }
  t->n = 0;      // (not a table until it has been enqueued)
  hipError_t rc = hipSuccess;
  if( !t->dev ) rc = hipMalloc( (void**) &t->dev, VVR_RESAMPLE_TABLE_BYTES );
  if( rc == hipSuccess && !t->host ) rc = hipHostMalloc( (void**) &t->host, VVR_RESAMPLE_TABLE_BYTES, hipHostMallocDefault );
  if( rc == hipSuccess && !t->uploaded ) rc = hipEventCreateWithFlags( &t->uploaded, hipEventDisableTiming );
  else if( rc == hipSuccess ) rc = hipEventSynchronize( t->uploaded );
  if( rc != hipSuccess ) return rc;
  int16_t w[VVR_RESAMPLE_MAX_TAPS]; int first = 0, most = 0;
  uint32_t* words = (uint32_t*) t->host;
  for( int i = 0; i < m; i++ )
  {
    const int count = resample_taps_of( filter, n, m, phi, i, first, w );
    if( count <= 0 || first < 0 || first + count > n ) return hipErrorInvalidValue;      // (every tap inside the plane: what the kernel's loads rely on)
    words[i] = (uint32_t) first | (uint32_t) count << 16; most = std::max( most, count );
  }
  const size_t bytes = (size_t) m * 4 + (size_t) most * m * 2;
  if( bytes > VVR_RESAMPLE_TABLE_BYTES ) return hipErrorInvalidValue;
  int16_t* wt = (int16_t*) ( words + m );
  memset( wt, 0, (size_t) most * m * 2 );
  for( int i = 0; i < m; i++ ) { const int count = resample_taps_of( filter, n, m, phi, i, first, w ); for( int k = 0; k < count; k++ ) wt[(size_t) k * m + i] = w[k]; }
  rc = hipMemcpyAsync( t->dev, t->host, bytes, hipMemcpyHostToDevice, s );
  if( rc == hipSuccess ) rc = hipEventRecord( t->uploaded, s );
  if( rc != hipSuccess ) return rc;
  t->n = n; t->m = m; t->phi = phi; t->filter = filter; t->taps = most; t->used = ++c->resampleUses;
  tab = (const uint32_t*) t->dev; taps = most;
  return hipSuccess;
}
}   // namespace

extern "C" {

// (a call that fails while a request is being enqueued: `who` is the submit call, s the output stream - drained, the entry's buffers may be reused at once)
#define OQCHK( call ) do { hipError_t e_ = ( call ); if( e_ != hipSuccess ) { c->setError( std::string( who ) + ": " #call ": " + hipGetErrorString( e_ ) ); hipStreamSynchronize( s ); return VVR_ERR_DEVICE; } } while( 0 )

// vvr_output_submit (bt == NULL) and vvr_output_submit_batch: one request path.  A batch is the single request with `count` regions where that has
// one: the checks, the context state, the tap tables and the launches are the request's; a region adds a row of the table of origins (three words:
// its sample offset in each plane of the slot, uploaded through the entry's pinned memory on the output stream like the grain's words) and its
// place in the entry's buffers and in the destination - plane k of region i at i * step from plane k of region 0.
#define VVR_OUT_BATCH_SCRATCH_MAX ( (size_t) 512 << 20 )
static_assert( sizeof( vvr_output_batch ) == 40 && offsetof( vvr_output_batch, count ) == 4 && offsetof( vvr_output_batch, origin ) == 8 && offsetof( vvr_output_batch, batch_stride_bytes ) == 16,
               "vvr_output_batch is part of the ABI" );
static int outputSubmit( vvr_context* c, const vvr_output_request* rq, const vvr_output_batch* bt, const char* const who )
{
  if( !c || !rq ) return VVR_ERR_PARAMETER;
  auto outRefuse = [who]( vvr_context* c, const std::string& why ) { return ::outRefuse( c, why.c_str(), who ); };
  // ---- 1. the request
  if( rq->struct_size != sizeof( vvr_output_request ) ) return outRefuse( c, "struct_size is not sizeof( vvr_output_request )" );
  const int count = bt ? (int) bt->count : 1;
  if( bt )
  {
    if( bt->struct_size != sizeof( vvr_output_batch ) ) return outRefuse( c, "struct_size is not sizeof( vvr_output_batch )" );
    if( bt->count < 1 || bt->count > VVR_OUT_BATCH_MAX ) return outRefuse( c, "count must be 1 .. 256 (VVR_OUT_BATCH_MAX)" );
    if( !bt->origin ) return outRefuse( c, "origin is NULL" );
    if( rq->x | rq->y ) return outRefuse( c, "x and y of the request must be 0 (a region's window starts at its origin)" );
    if( rq->grain ) return outRefuse( c, "grain is not offered for a batch (the seed chain is defined per frame)" );
  }
  const int slot = rq->slot, bd = c->cfg.bit_depth, nc = c->cfg.chroma_format ? 3 : 1, x = rq->x, y = rq->y, w = rq->w, h = rq->h;
  if( slot < 0 || slot >= (int) c->slots.size() || !c->slots[slot].p[0] ) return outRefuse( c, "no such slot" );
  // the RGB formats: three planes (RGB8, RGB16, RGBF16, RGBF32) or one plane of pixels (`inter`); px: bytes of a sample of a plane, or of a pixel
  const bool inter = rq->format >= VVR_OUT_RGBA8 && rq->format <= VVR_OUT_RGBA16F;
  const bool rgb = rq->format == VVR_OUT_RGB8 || rq->format == VVR_OUT_RGB16 || rq->format == VVR_OUT_RGBF16 || rq->format == VVR_OUT_RGBF32 || inter;
  const bool rgb8 = rq->format == VVR_OUT_RGB8 || rq->format == VVR_OUT_RGBA8 || rq->format == VVR_OUT_BGRA8 || rq->format == VVR_OUT_RGB24 || rq->format == VVR_OUT_BGR24;      // (the values VVR_OUT_RGB8 stores)
  const int px = rq->format == VVR_OUT_RGB8 ? 1 : rq->format == VVR_OUT_RGB24 || rq->format == VVR_OUT_BGR24 ? 3 : rq->format == VVR_OUT_RGBA16F ? 8 : rq->format == VVR_OUT_RGB16 || rq->format == VVR_OUT_RGBF16 ? 2 : 4;
  // the Y'CbCr formats at 4:4:4 / 4:2:2 (k_output_yuv): three planes, or one packed plane (`yuvOne`); yuv8: the sample as a byte
  const bool yuv = rq->format >= VVR_OUT_YUV444P8 && rq->format <= VVR_OUT_Y410;
  const bool yuv444 = rq->format == VVR_OUT_YUV444P8 || rq->format == VVR_OUT_YUV444P16 || rq->format == VVR_OUT_Y410, yuvOne = yuv && rq->format >= VVR_OUT_UYVY;
  const bool yuv8 = rq->format == VVR_OUT_YUV444P8 || rq->format == VVR_OUT_YUV422P8 || rq->format == VVR_OUT_UYVY || rq->format == VVR_OUT_YUY2;
  if( rq->format > VVR_OUT_PACKED10 && rq->format != VVR_OUT_NV12 && rq->format != VVR_OUT_P010 && !rgb && !yuv ) return outRefuse( c, "unknown format" );
  if( bt && !rgb ) return outRefuse( c, "a batch takes the ten R'G'B' formats (VVR_OUT_RGB8 ... VVR_OUT_RGBA16F)" );
  if( rq->job < -1 ) return outRefuse( c, "job must be a job id or -1" );
  const bool packed = rq->format == VVR_OUT_PACKED10, semi = rq->format == VVR_OUT_NV12 || rq->format == VVR_OUT_P010, grain = rq->grain != 0, scaled = rq->out_w != 0 || rq->out_h != 0;
  const bool narrow = rq->format == VVR_OUT_PLANAR8 || rq->format == VVR_OUT_NV12 || yuv8;
  const bool reduce = narrow && bd > 8;      // (accepted under a mode of vvr_set_output_narrowing alone: k_output_narrow or k_output_yuv reduces at its store)
  const bool viaTmp = packed || semi || rgb || yuv || reduce;      // k_output_frame / k_output_narrow / k_output_rgb / k_output_yuv makes the format: the stages before it store 16-bit samples into `tmp`
  const int bps = narrow ? 1 : rgb ? px : 2, nOut = semi ? 2 : inter || yuvOne ? 1 : yuv ? 3 : nc;
  int outMatrix = 0, outFullRange = 0;      // (the colour description: looked at here for the refusal, taken under mu where the request is accepted)
  if( rgb )
  {
    { std::lock_guard<std::mutex> lk( c->mu ); outMatrix = c->outMatrix; outFullRange = c->outFullRange; }
    if( nc == 1 ) return outRefuse( c, "RGB output of a 4:0:0 context: there is no chroma to convert" );
    if( !outMatrix ) return outRefuse( c, "RGB output with no colour description set (vvr_set_output_colour)" );
    if( bd < 8 || bd > 10 ) return outRefuse( c, "RGB output needs a bit depth of 8, 9 or 10" );
    if( scaled && ( ( rq->out_w | rq->out_h ) & 1 ) ) return outRefuse( c, "RGB output needs an even out_w and out_h (one 4:2:0 frame is converted)" );
  }
  if( semi && nc == 1 ) return outRefuse( c, "semi-planar output of a 4:0:0 context: there is no chroma to interleave" );
  if( yuv && nc == 1 ) return outRefuse( c, "4:2:2 / 4:4:4 output of a 4:0:0 context: there is no chroma to upsample" );
  if( rq->format == VVR_OUT_P010 && ( bd < 8 || bd > 10 ) ) return outRefuse( c, "P010 output needs a bit depth of 8, 9 or 10" );
  static const char* const noNarrowing = "8-bit output of a stream with more than 8 bits per sample (only narrowing of 8-bit content, vvdecimpl.cpp:853)";
  int outNarrow = 0, outNarrowPhase = 0;      // (the narrowing: looked at here for the refusal, taken under mu where the request is accepted)
  if( reduce )
  {
    { std::lock_guard<std::mutex> lk( c->mu ); outNarrow = c->outNarrow; }
    if( !outNarrow || bd > 10 ) return outRefuse( c, noNarrowing );
  }
  if( packed && bd != 8 && bd != 10 ) return outRefuse( c, "packed 10-bit output needs a bit depth of 8 or 10 (vvdecHelper.h:106-248)" );
  if( yuv && ( bd < 8 || bd > 10 ) ) return outRefuse( c, "4:2:2 / 4:4:4 output needs a bit depth of 8, 9 or 10" );
  if( yuv && scaled && ( ( rq->out_w | rq->out_h ) & 1 ) ) return outRefuse( c, "4:2:2 / 4:4:4 output needs an even out_w and out_h (one 4:2:0 frame is upsampled)" );
  const DevPlanes d = pictureIn( c, slot );
  if( x < 0 || y < 0 || w <= 0 || h <= 0 || x + w > d.w[0] || y + h > d.h[0] || ( nc > 1 && ( ( x | y | w | h ) & 1 ) ) ) return outRefuse( c, "window outside the picture, or odd in 4:2:0" );
  for( int i = 0; bt && i < count; i++ )
  {
    const int ox = bt->origin[2 * i], oy = bt->origin[2 * i + 1];
    if( ox < 0 || oy < 0 || ox > d.w[0] - w || oy > d.h[0] - h || ( nc > 1 && ( ( ox | oy ) & 1 ) ) )
      return outRefuse( c, "region " + std::to_string( i ) + ": window outside the picture, or odd in 4:2:0" );
  }
  if( grain )
  {
    if( !c->grainBank ) return outRefuse( c, "no film grain bank set" );
    if( bd != 8 && bd != 10 ) return outRefuse( c, "film grain needs a bit depth of 8 or 10 (FilmGrainImpl::set_depth)" );
    if( w <= 128 ) return outRefuse( c, "film grain needs a frame wider than 128 samples (FilmGrainImpl::add_grain_block)" );
  }
  // the filter out_w / out_h resample with: the one that is set now, read once (0: the reference's DCTIF, k_rescale, and its range)
  int resample = 0;
  if( scaled ) { std::lock_guard<std::mutex> lk( c->mu ); resample = c->outResample; }
  int pw[3], ph[3], ow[3], oh[3], outRows[3]; bool resc[3] = { false, false, false }, anyResc = false;
  size_t rowBytes[3] = { 0, 0, 0 };
  for( int k = 0; k < nc; k++ )
  {
    const int s = k ? 1 : 0;
    pw[k] = w >> s; ph[k] = h >> s; ow[k] = scaled ? rq->out_w >> s : pw[k]; oh[k] = scaled ? rq->out_h >> s : ph[k];
    if( scaled && resample && ( ow[k] <= 0 || oh[k] <= 0 || !resample_axis_ok( pw[k], ow[k] ) || !resample_axis_ok( ph[k], oh[k] ) ) )
      return outRefuse( c, "under vvr_set_output_resampling window and output sides must be 1..8192, the output's within 1/64 .. 8 times the window's in every plane" );
    if( scaled && !resample && ( ow[k] <= 0 || oh[k] <= 0 || ow[k] > 8192 || oh[k] > 8192 || pw[k] > 8 * ow[k] || ph[k] > 8 * oh[k] || ow[k] > 8 * pw[k] || oh[k] > 8 * ph[k] ) )
      return outRefuse( c, "output sides must be 1..8192 and within 1/8 .. 8 times the window's" );
    resc[k] = ow[k] != pw[k] || oh[k] != ph[k]; anyResc |= resc[k];
    if( packed && ( ow[k] & 3 ) ) return outRefuse( c, "packed 10-bit output needs plane widths that are multiples of 4 (four samples in five bytes)" );
    rowBytes[k] = packed ? (size_t) ow[k] / 4 * 5 : (size_t) ow[rgb ? 0 : k] * bps * ( semi && k ? 2 : 1 );      // (semi-planar plane 1: Cb and Cr interleaved; RGB: every plane at the luma size)
    outRows[k] = oh[rgb ? 0 : k];
    if( yuv )      // (every plane has the luma rows; the chroma planes of the planar 4:2:2 formats half the luma samples of a row)
    {
      const size_t W0 = (size_t) ow[0];
      rowBytes[k] = rq->format == VVR_OUT_V210 ? ( W0 + 5 ) / 6 * 16 : rq->format == VVR_OUT_Y210 || rq->format == VVR_OUT_Y410 ? W0 * 4 : yuvOne ? W0 * 2 : ( yuv444 || !k ? W0 : W0 >> 1 ) * ( yuv8 ? 1 : 2 );
      outRows[k] = oh[0];
    }
    if( k < nOut && ( !rq->dst[k] || rq->dst_stride_bytes[k] < rowBytes[k] ) ) return outRefuse( c, "missing plane or stride below the output's row" );
  }
  // a batch: plane k of region i lies i * bstride[k] behind plane k of region 0, regions do not overlap in the destination; span[k]: from the
  // first byte of plane k of region 0 to the last of the last region (a single request: the plane's extent)
  size_t extent[3] = { 0, 0, 0 }, span[3] = { 0, 0, 0 }, bstride[3] = { 0, 0, 0 };
  for( int k = 0; k < nOut; k++ )
  {
    extent[k] = (size_t) ( outRows[k] - 1 ) * rq->dst_stride_bytes[k] + rowBytes[k];
    if( bt )
    {
      bstride[k] = bt->batch_stride_bytes[k];
      if( bstride[k] < extent[k] ) return outRefuse( c, "batch_stride_bytes below the plane's extent ( rows - 1 ) * dst_stride_bytes + row bytes: regions would overlap in the destination" );
    }
    span[k] = (size_t) ( count - 1 ) * bstride[k] + extent[k];
  }
  hipSetDevice( c->device );
  // ---- 2. a ring entry; the picture has been handed to the device
  OutEntry* e = nullptr;
  hipEvent_t jobDone = nullptr; int jobFailed = VVR_OK;
  std::unique_lock<std::mutex> lk( c->mu );
  { const int rc = outAcquire( c, who, slot, rq->job, rq->blocking != 0, lk, e, jobDone, jobFailed ); if( rc != VVR_OK ) return rc; }
  hipStream_t s = c->outQStream;
  // ---- where the planes go: device memory the context knows (every plane wholly inside a range), or the host
  int devPlanes = 0;
  for( int k = 0; k < nOut; k++ )
  {
    const char* b = (const char*) rq->dst[k];
    for( const DevRange& r : c->devRanges )
    {
      if( b >= r.p && b + span[k] <= r.p + r.n ) { devPlanes++; break; }
      if( b < r.p + r.n && b + span[k] > r.p ) { c->setError( std::string( who ) + ": a destination plane lies partly inside a device range (vvr_device_alloc / vvr_device_register)" ); return VVR_ERR_PARAMETER; }
    }
  }
  if( devPlanes && devPlanes != nOut ) { c->setError( std::string( who ) + ": destination planes in device memory mixed with planes in host memory" ); return VVR_ERR_PARAMETER; }
  const bool devDst = devPlanes != 0;
  if( rgb ) { outMatrix = c->outMatrix; outFullRange = c->outFullRange; }      // (what is set now, behind the waits above: a description cannot be unset)
  // the narrowing the request takes: the one that is set now (it can be unset: the request is refused then, no entry has been taken); the four
  // constants of the 2 x 2 cell, the phase folded in, go with the request as kernel arguments - the three modes are one kernel path
  NarrowArgs na; memset( &na, 0, sizeof( na ) );
  if( reduce )
  {
    outNarrow = c->outNarrow; outNarrowPhase = c->outNarrowPhase;
    if( !outNarrow ) { c->setError( std::string( who ) + ": " + noNarrowing ); return VVR_ERR_PARAMETER; }
    static const int M[2][2] = { { 0, 2 }, { 3, 1 } };
    na.s = bd - 8; na.maxVal = ( 1 << bd ) - 1;
    for( int j = 0; j < 2; j++ )
    {
      uint32_t a[2];
      for( int i = 0; i < 2; i++ )
        a[i] = outNarrow == VVR_NARROW_TRUNCATE ? 0 : outNarrow == VVR_NARROW_ROUND ? 1u << ( na.s - 1 ) : (uint32_t) M[( j + ( outNarrowPhase >> 1 & 1 ) ) & 1][( i + ( outNarrowPhase & 1 ) ) & 1] >> ( 2 - na.s );
      na.cell[j] = a[0] | a[1] << 16;
    }
  }
  // the colour transform the request takes: the one that is set now.  Its matrix goes with the request as kernel arguments; its tables, when
  // they have changed, are refreshed on the output stream ahead of the request's kernel - behind the kernels of the requests in flight
  const bool xf = rgb && c->xform, xfUpload = xf && c->xformStale;
  // ... and the 3-D LUT, by the same rule: its size goes with the request, its nodes are refreshed on the output stream when they have changed
  const int lutN = rgb ? c->lutN : 0;
  const bool lutUpload = lutN && c->lutStale;
  const size_t lutBytes = (size_t) lutN * lutN * lutN * 8;
  // the normalisation a VVR_OUT_RGBF32 request takes: the one that is set now, as scale and bias computed in double and rounded once (vvr.h)
  float nscale[3], nbias[3];
  for( int k = 0; k < 3; k++ )
  {
    const double M = xf || lutN ? 65535. : (double) ( ( 1 << bd ) - 1 );
    nscale[k] = c->outNorm ? (float) ( 1.0 / ( M * (double) c->outStd[k] ) ) : (float) ( 1.0 / M );
    nbias[k] = c->outNorm ? (float) ( -(double) c->outMean[k] / (double) c->outStd[k] ) : 0.f;
  }
  int xm[3][3] = { { 0, 0, 0 }, { 0, 0, 0 }, { 0, 0, 0 } };
  if( xf ) memcpy( xm, c->xform->m, sizeof( xm ) );
  // ---- the entry's buffers: the output's planes; the 16-bit planes of a grained frame that goes on (A) and of a rescaled plane that is packed (B); the words.
  // A batch: plane k of its regions at off[k] + i * step[k] in `dev`, the rescaled planes of its regions back to back at offB[k], the
  // horizontal results of the two-launch form back to back at offH, the table of origins behind the words
  const bool grainTmp = grain && ( viaTmp || anyResc );
  size_t total = 0, tmpBytes = 0, offA[3] = { 0, 0, 0 }, offB[3] = { 0, 0, 0 }, step[3] = { 0, 0, 0 };
  bool direct = true, kdirect[3] = { false, false, false };      // kdirect: k_output_frame stores the plane straight into the caller's device memory
  for( int k = 0; k < nOut; k++ )
  {
    const bool frameStores = viaTmp || !( ( grain && !grainTmp ) || resc[k] );      // (else k_film_grain / k_rescale store the plane themselves)
    kdirect[k] = devDst && frameStores && rq->dst_stride_bytes[k] == rowBytes[k] && ( (uintptr_t) rq->dst[k] & 31 ) == 0 && ( bstride[k] & 31 ) == 0;
    e->off[k] = total; e->rowBytes[k] = rowBytes[k]; e->rows[k] = outRows[k]; e->dst[k] = rq->dst[k]; e->dstStride[k] = rq->dst_stride_bytes[k]; e->extent[k] = span[k];
    step[k] = outRegion( rowBytes[k] * outRows[k] ); e->step[k] = step[k]; e->bstride[k] = bstride[k];
    if( !kdirect[k] ) total += (size_t) count * step[k];
    direct = direct && ( devDst || c->pinned.contains( rq->dst[k], span[k] ) );
  }
  for( int k = 0; k < nc; k++ )
  {
    if( grainTmp ) { offA[k] = tmpBytes; tmpBytes += outRegion( (size_t) pw[k] * ph[k] * 2 ); }
    if( resc[k] && viaTmp ) { offB[k] = tmpBytes; tmpBytes += outRegion( (size_t) count * ow[k] * oh[k] * 2 ); }
  }
  // (... and the horizontal results of a plane that k_output_resample takes in two launches: one region, the planes use it in turn on the stream)
  size_t offH = tmpBytes, bytesH = 0;
  for( int k = 0; k < nc; k++ ) if( resample && resc[k] && resample_two_launches( ph[k], oh[k] ) ) bytesH = std::max( bytesH, (size_t) count * ph[k] * ow[k] * sizeof( int ) );
  tmpBytes += alignUp( bytesH, 256 );
  if( bt && total + tmpBytes > VVR_OUT_BATCH_SCRATCH_MAX )
  { c->setError( std::string( who ) + ": the batch's device buffers in the ring entry (outputs not stored directly, resampled frames, horizontal results) would exceed the limit of 512 MiB: submit fewer regions per request" ); return VVR_ERR_PARAMETER; }
  outTake( c, e, slot, rq->job, jobFailed ); e->nc = nOut; e->count = count;
  if( jobFailed != VVR_OK ) { e->state = OQ_FLIGHT; return e->ticket; }      // (nothing to run: the request fails with the job's status)
  const int nbx = ( w + 15 ) / 16, nby = ( h + 15 ) / 16;
  const size_t wordsBytes = grain ? (size_t) nbx * nby * sizeof( uint32_t ) : 0, wordsOff = tmpBytes, hostWordsOff = direct ? 0 : total;
  tmpBytes += alignUp( wordsBytes, 256 );
  const size_t tabBytes = bt ? (size_t) count * 3 * sizeof( uint32_t ) : 0, tabOff = tmpBytes;
  tmpBytes += alignUp( tabBytes, 256 );
  const size_t hostBankOff = hostWordsOff + alignUp( wordsBytes, 256 );      // (a bank that changed travels through the entry's pinned memory: the context's copy may change while the upload is in flight)
  const size_t hostXformOff = hostBankOff + ( grain && c->grainBankStale ? alignUp( sizeof( vvr_film_grain_bank ), 256 ) : 0 );      // (... and so do the tables of a transform that changed)
  // (... and the nodes of a LUT that changed: up to 2.2 MB more of the entry's pinned staging, grown below once per entry like the staging of a
  // larger output - the device copy is never reallocated, the staging is only ever enlarged)
  const size_t hostLutOff = hostXformOff + ( xfUpload ? alignUp( sizeof( vvr_output_transform ), 256 ) : 0 );
  const size_t hostTabOff = hostLutOff + ( lutUpload ? alignUp( lutBytes, 256 ) : 0 );      // (... and the table of a batch's origins)
  if( outGrow( e->dev, e->devCap, total, false ) != VVR_OK || outGrow( e->tmp, e->tmpCap, tmpBytes, false ) != VVR_OK || outGrow( e->host, e->hostCap, hostTabOff + tabBytes, true ) != VVR_OK )
  { c->setError( std::string( who ) + ": out of device or pinned memory" ); return VVR_ERR_DEVICE; }
  e->direct = direct; e->devDst = devDst;
  // ---- 3. behind the picture (or the slot's users) on the device, 4. the kernels.  mu stays held up to the registration of the `read` event: a
  // picture committed meanwhile that overwrites the slot must find it
  OQCHK( outOrder( c, e, slot, rq->job, jobDone ) );
  struct Cur { const pel_t* p; int stride; bool inOut; } cur[3];
  for( int k = 0; k < nc; k++ ) { const int sh = k ? 1 : 0; cur[k].p = d.p[k] + (size_t) ( y >> sh ) * d.stride[k] + ( x >> sh ); cur[k].stride = d.stride[k]; cur[k].inOut = false; }
  // a batch: the table of origins - per region its sample offset in each plane of the slot - through the entry's pinned memory; the kernels
  // that read the slot take it (useTab), those behind them read the regions' planes in `tmp` back to back
  const uint32_t* regionTab = nullptr;
  if( bt )
  {
    uint32_t* tab = (uint32_t*) ( e->host + hostTabOff );
    for( int i = 0; i < count; i++ )
      for( int k = 0; k < 3; k++ )
      {
        const int sh = k ? 1 : 0, kk = k < nc ? k : 0;
        tab[3 * i + k] = (uint32_t) ( (size_t) ( bt->origin[2 * i + 1] >> sh ) * d.stride[kk] + ( bt->origin[2 * i] >> sh ) );
      }
    OQCHK( hipMemcpyAsync( e->tmp + tabOff, tab, tabBytes, hipMemcpyHostToDevice, s ) );
    regionTab = (const uint32_t*) ( e->tmp + tabOff );
  }
  uint32_t nextSeed = c->grainSeed;
  if( grain )
  {
    uint32_t* words = (uint32_t*) ( e->host + hostWordsOff );
    nextSeed = grain_words( c->grainSeed, nbx, nby, words );
    if( !c->grainBankDev ) OQCHK( hipMalloc( &c->grainBankDev, sizeof( vvr_film_grain_bank ) ) );
    if( c->grainBankStale )
    {
      memcpy( e->host + hostBankOff, c->grainBank.get(), sizeof( vvr_film_grain_bank ) );
      OQCHK( hipMemcpyAsync( c->grainBankDev, e->host + hostBankOff, sizeof( vvr_film_grain_bank ), hipMemcpyHostToDevice, s ) );
    }
    OQCHK( hipMemcpyAsync( e->tmp + wordsOff, words, wordsBytes, hipMemcpyHostToDevice, s ) );
    FilmGrainParams p;
    for( int k = 0; k < 3; k++ )
    {
      p.src[k] = k < nc ? cur[k].p : nullptr; p.stride[k] = d.stride[k]; p.w[k] = w >> ( k ? 1 : 0 ); p.h[k] = h >> ( k ? 1 : 0 );
      p.dstOff[k] = k < nc ? ( grainTmp ? offA[k] : e->off[k] ) : 0;
    }
    p.bank = (const vvr_film_grain_bank*) c->grainBankDev; p.words = (const uint32_t*) ( e->tmp + wordsOff ); p.nbx = nbx;
    p.numComp = nc; p.bs = bd - 8; p.scaleShift = c->grainBank->shift + 6 - p.bs; p.bytesPerSample = grainTmp ? 2 : bps;
    launch_film_grain( s, p, grainTmp ? e->tmp : e->dev );
    for( int k = 0; k < nc; k++ )
      if( grainTmp ) { cur[k].p = (const pel_t*) ( e->tmp + offA[k] ); cur[k].stride = pw[k]; } else cur[k].inOut = true;
  }
  if( resample && anyResc )
  {
    // vvr_set_output_resampling: k_output_resample where k_rescale stands below, with the same two store forms; the tap tables of the axes
    // from the context's cache (phi: 2 for luma and for chroma whose collocated bit is 0, 1 for chroma whose bit is 1)
    double bytes = 0; int launches = 0;
    ResampleParams rp[3];
    for( int k = 0; k < nc; k++ )
    {
      if( !resc[k] ) continue;
      ResampleParams& p = rp[k];
      p.src = cur[k].p; p.stride = cur[k].stride; p.w = pw[k]; p.h = ph[k]; p.outW = ow[k]; p.outH = oh[k];
      p.maxVal = ( 1 << bd ) - 1; p.bytesPerSample = viaTmp ? 2 : bps;
      OQCHK( resampleTable( c, s, resample, pw[k], ow[k], k && ( rq->collocated & 1 ) ? 1 : 2, p.tabX, p.tapsX ) );
      OQCHK( resampleTable( c, s, resample, ph[k], oh[k], k && ( rq->collocated & 2 ) ? 1 : 2, p.tabY, p.tapsY ) );
      bytes += ( (double) pw[k] * ph[k] * 2 + (double) ow[k] * oh[k] * p.bytesPerSample ) * count; launches++;      // (a request's planes count one launch each, in one or two parts - whatever the number of regions)
    }
    outTimeBegin( c, s, e->timed0, e->timing0, K_OUTPUT_RESAMPLE, bytes );
    for( int k = 0; k < nc; k++ )
    {
      if( !resc[k] ) continue;
      PlaneRegions rg;      // (a batch is an RGB request: its planes go on to k_output_rgb through `tmp`)
      rg.count = count; rg.comp = k; rg.srcOff = regionTab; rg.dstStep = bt ? (size_t) ow[k] * oh[k] * 2 : 0; rg.hStep = bt ? (size_t) ph[k] * ow[k] : 0;
      launch_output_resample( s, rp[k], viaTmp ? e->tmp + offB[k] : e->dev + e->off[k], e->tmp + offH, rg );
      if( viaTmp ) { cur[k].p = (const pel_t*) ( e->tmp + offB[k] ); cur[k].stride = ow[k]; } else cur[k].inOut = true;
    }
    if( e->timed0 ) hipEventRecord( e->timing0.b, s );
    e->rescales = launches;
  }
  for( int k = 0; k < nc; k++ )
  {
    if( !resc[k] || resample ) continue;
    // (as vvr_read_output_scaled: the component's subsampling, luma always collocated)
    const bool luma = k == 0;
    const int cs = luma ? 0 : 1, colX = luma ? 1 : rq->collocated & 1, colY = luma ? 1 : ( rq->collocated >> 1 ) & 1, fracShift = luma ? 4 : 5;
    RescaleParams p;
    p.src = cur[k].p; p.stride = cur[k].stride; p.w = pw[k]; p.h = ph[k]; p.outW = ow[k]; p.outH = oh[k];
    p.luma = luma; p.maxVal = ( 1 << bd ) - 1; p.bytesPerSample = viaTmp ? 2 : bps;
    int scale;
    rescale_axis( pw[k], ow[k], cs, colX, fracShift, scale, p.addX, p.shiftX ); p.stepX = scale << cs;
    rescale_axis( ph[k], oh[k], cs, colY, fracShift, scale, p.addY, p.shiftY ); p.stepY = scale << cs;
    PlaneRegions rg;
    rg.count = count; rg.comp = k; rg.srcOff = regionTab; rg.dstStep = bt ? (size_t) ow[k] * oh[k] * 2 : 0;
    launch_rescale( s, p, viaTmp ? e->tmp + offB[k] : e->dev + e->off[k], rg );
    if( viaTmp ) { cur[k].p = (const pel_t*) ( e->tmp + offB[k] ); cur[k].stride = ow[k]; } else cur[k].inOut = true;
  }
  OutputFrameParams fp; memset( &fp, 0, sizeof( fp ) );
  double frameBytes = 0;
  for( int k = 0; k < nc && !rgb && !yuv; k++ )
    if( !cur[k].inOut )
    {
      fp.src[k] = cur[k].p; fp.stride[k] = cur[k].stride; frameBytes += (double) ow[k] * oh[k] * 2 + ( k < nOut ? (double) rowBytes[k] * oh[k] : 0. );
      if( k < nOut ) { fp.w[k] = semi && k ? 2 * ow[k] : ow[k]; fp.h[k] = oh[k]; fp.dstOff[k] = e->off[k]; fp.direct[k] = kdirect[k] ? (uint8_t*) rq->dst[k] : nullptr; }
    }
  fp.format = rq->format; fp.shift = packed ? 10 - bd : ( rq->format == VVR_OUT_P010 ? 16 - bd : 0 );
  if( frameBytes > 0 )
  {
    outTimeBegin( c, s, e->timed, e->timing, reduce ? K_OUTPUT_NARROW : K_OUTPUT_FRAME, frameBytes );
    if( reduce ) launch_output_narrow( s, fp, na, e->dev ); else launch_output_frame( s, fp, e->dev );
    if( e->timed ) hipEventRecord( e->timing.b, s );
  }
  if( rgb )
  {
    // the frame as it stands - the slot's window, or the grained / rescaled planes in `tmp` - converted in one launch
    OutputRgbParams rp; memset( &rp, 0, sizeof( rp ) );
    for( int k = 0; k < 3; k++ ) { rp.src[k] = cur[k].p; rp.stride[k] = cur[k].stride; rp.dstOff[k] = k < nOut ? e->off[k] : 0; rp.direct[k] = k < nOut && kdirect[k] ? (uint8_t*) rq->dst[k] : nullptr; }
    rp.w = ow[0]; rp.h = oh[0]; rp.collocated = rq->collocated & 3;
    rp.format = rq->format == VVR_OUT_BGRA8 ? VVR_OUT_RGBA8 : rq->format == VVR_OUT_BGR24 ? VVR_OUT_RGB24 : rq->format;      // (the class the kernel is compiled for)
    rp.swapRB = rq->format == VVR_OUT_BGRA8 || rq->format == VVR_OUT_BGR24;
    rgb_coefficients( outMatrix, outFullRange, bd, xf || lutN ? bd : rgb8 ? 8 : rq->format == VVR_OUT_RGB10A2 ? 10 : bd, rp );
    for( int k = 0; k < 3; k++ ) { rp.nscale[k] = nscale[k]; rp.nbias[k] = nbias[k]; }
    if( xf )
    {
      if( !c->xformDev ) OQCHK( hipMalloc( &c->xformDev, sizeof( vvr_output_transform ) ) );
      if( xfUpload )
      {
        memcpy( e->host + hostXformOff, c->xform.get(), sizeof( vvr_output_transform ) );
        OQCHK( hipMemcpyAsync( c->xformDev, e->host + hostXformOff, sizeof( vvr_output_transform ), hipMemcpyHostToDevice, s ) );
      }
      rp.xform = (const vvr_output_transform*) c->xformDev; memcpy( rp.xm, xm, sizeof( xm ) );
      rp.inv = 1.0f / 65535.0f;
    }
    if( lutN )
    {
      if( !c->lutDev ) OQCHK( hipMalloc( &c->lutDev, (size_t) VVR_LUT3D_MAX * VVR_LUT3D_MAX * VVR_LUT3D_MAX * 8 ) );
      if( lutUpload )
      {
        memcpy( e->host + hostLutOff, c->lut.data(), lutBytes );
        OQCHK( hipMemcpyAsync( c->lutDev, e->host + hostLutOff, lutBytes, hipMemcpyHostToDevice, s ) );
      }
      rp.lut = (const uint16_t*) c->lutDev; rp.lutN = lutN; rp.lutShift = lutN == 17 ? 12 : lutN == 33 ? 11 : 10;
      rp.lutWiden = (uint32_t) ( ( 1ull << 39 ) / (unsigned) ( ( 1 << bd ) - 1 ) + 1 );
      rp.inv = 1.0f / 65535.0f;
    }
    // the regions of a batch: their windows of the slot through the table, or - every plane is rescaled or none: w, h, out_w, out_h are even -
    // their rescaled planes in `tmp` back to back; their outputs a step apart in the entry's scratch or in the caller's device memory
    RgbRegions rg; rg.count = count; rg.srcOff = anyResc ? nullptr : regionTab;
    for( int k = 0; k < 3; k++ ) { rg.srcStep[k] = bt && anyResc ? (size_t) ow[k] * oh[k] : 0; rg.dstStep[k] = !bt || k >= nOut ? 0 : kdirect[k] ? bstride[k] : step[k]; }
    outTimeBegin( c, s, e->timed, e->timing, K_OUTPUT_RGB, (double) rp.w * rp.h * ( 3. + (double) nOut * px ) * count );      // (read: 2 bytes of luma, 2 x 2 / 4 of chroma; written: the planes, or the pixel)
    launch_output_rgb( s, rp, e->dev, rg );
    if( e->timed ) hipEventRecord( e->timing.b, s );
  }
  if( yuv )
  {
    // the frame as it stands, as the RGB formats take it, with the chroma upsampled and the format's store in one launch
    OutputYuvParams yp; memset( &yp, 0, sizeof( yp ) );
    double written = 0;
    for( int k = 0; k < 3; k++ ) { yp.src[k] = cur[k].p; yp.stride[k] = cur[k].stride; yp.dstOff[k] = k < nOut ? e->off[k] : 0; yp.direct[k] = k < nOut && kdirect[k] ? (uint8_t*) rq->dst[k] : nullptr; }
    for( int k = 0; k < nOut; k++ ) written += (double) rowBytes[k] * outRows[k];
    yp.w = ow[0]; yp.h = oh[0]; yp.collocated = rq->collocated & 3; yp.format = rq->format; yp.maxVal = ( 1 << bd ) - 1;
    yp.shift = rq->format == VVR_OUT_Y210 ? 16 - bd : rq->format == VVR_OUT_V210 || rq->format == VVR_OUT_Y410 ? 10 - bd : 0;
    yp.narrow = na;      // (s == 0 unless a byte format leaves a context of 9 or 10 bits: the kernel's NARROW variants, counted under k_output_yuv)
    outTimeBegin( c, s, e->timed, e->timing, K_OUTPUT_YUV, (double) yp.w * yp.h * 3. + written );      // (read: 2 bytes of luma, 2 x 2 / 4 of chroma; written: the planes)
    launch_output_yuv( s, yp, e->dev );
    if( e->timed ) hipEventRecord( e->timing.b, s );
  }
  OQCHK( hipGetLastError() );
  OQCHK( hipEventRecord( e->read, s ) );
  c->slotExt[slot].push_back( e->read );
  e->state = OQ_FLIGHT; e->queued = true;
  if( grain ) { c->grainBankStale = false; c->grainSeed = nextSeed; }      // (the chain advances at submit, for an accepted request only)
  if( xfUpload ) c->xformStale = false;
  if( lutUpload ) c->lutStale = false;
  const int ticket = e->ticket;
  lk.unlock();
  // ---- the result's way to the host: exactly the output's bytes
  hipError_t ce = hipSuccess;
  for( int k = 0; k < nOut && ce == hipSuccess && bt; k++ )
  {
    // a batch: pageable destinations take the entry's planes of all regions as they lie, in one copy (vvr_output_wait moves the rows); a pinned
    // or device plane whose rows are back to back takes its regions as the rows of one 2-D copy, any other one a 2-D copy per region
    const hipMemcpyKind kind = devDst ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    const size_t planeBytes = rowBytes[k] * outRows[k];
    if( devDst && kdirect[k] ) continue;
    if( !devDst && !direct ) ce = hipMemcpyAsync( e->host + e->off[k], e->dev + e->off[k], (size_t) ( count - 1 ) * step[k] + planeBytes, kind, s );
    else if( rq->dst_stride_bytes[k] == rowBytes[k] ) ce = hipMemcpy2DAsync( rq->dst[k], bstride[k], e->dev + e->off[k], step[k], planeBytes, count, kind, s );
    else
      for( int i = 0; i < count && ce == hipSuccess; i++ )
        ce = hipMemcpy2DAsync( (char*) rq->dst[k] + (size_t) i * bstride[k], rq->dst_stride_bytes[k], e->dev + e->off[k] + (size_t) i * step[k], rowBytes[k], rowBytes[k], outRows[k], kind, s );
  }
  for( int k = 0; k < nOut && ce == hipSuccess && !bt; k++ )
  {
    if( devDst )      // (what k_output_frame has not stored itself: rows out of the entry's scratch at the caller's stride, on the device)
    {
      if( kdirect[k] ) continue;
      if( rq->dst_stride_bytes[k] == rowBytes[k] ) ce = hipMemcpyAsync( rq->dst[k], e->dev + e->off[k], rowBytes[k] * outRows[k], hipMemcpyDeviceToDevice, s );
      else ce = hipMemcpy2DAsync( rq->dst[k], rq->dst_stride_bytes[k], e->dev + e->off[k], rowBytes[k], rowBytes[k], outRows[k], hipMemcpyDeviceToDevice, s );
    }
    else if( !direct ) ce = hipMemcpyAsync( e->host + e->off[k], e->dev + e->off[k], rowBytes[k] * outRows[k], hipMemcpyDeviceToHost, s );
    else if( rq->dst_stride_bytes[k] == rowBytes[k] ) ce = hipMemcpyAsync( rq->dst[k], e->dev + e->off[k], rowBytes[k] * outRows[k], hipMemcpyDeviceToHost, s );
    else ce = hipMemcpy2DAsync( rq->dst[k], rq->dst_stride_bytes[k], e->dev + e->off[k], rowBytes[k], rowBytes[k], outRows[k], hipMemcpyDeviceToHost, s );
  }
  if( ce == hipSuccess ) ce = hipEventRecord( e->done, s );
  if( ce != hipSuccess )
  {
    // (the request stays accepted - its kernels have run, the chain has advanced - and fails from vvr_output_test / vvr_output_wait)
    hipStreamSynchronize( s );
    lk.lock(); e->rc = VVR_ERR_DEVICE; e->queued = false; c->setError( std::string( who ) + ": copy to the destination: " + hipGetErrorString( ce ) );
  }
  return ticket;
}

VVR_API int vvr_output_submit( vvr_context* c, const vvr_output_request* rq ) { return outputSubmit( c, rq, nullptr, "vvr_output_submit" ); }

VVR_API int vvr_output_submit_batch( vvr_context* c, const vvr_output_request* rq, const vvr_output_batch* bt )
{
  if( !c || !rq || !bt ) return VVR_ERR_PARAMETER;
  return outputSubmit( c, rq, bt, "vvr_output_submit_batch" );
}

VVR_API int vvr_hash_submit( vvr_context* c, const vvr_hash_request* rq )
{
  if( !c || !rq ) return VVR_ERR_PARAMETER;
  const char* const who = "vvr_hash_submit";
  // ---- 1. the request
  if( rq->struct_size != sizeof( vvr_hash_request ) ) return outRefuse( c, "struct_size is not sizeof( vvr_hash_request )", who );
  const int slot = rq->slot, method = rq->method, nc = c->cfg.chroma_format ? 3 : 1, len = method == VVR_HASH_MD5 ? 16 : method == VVR_HASH_CRC ? 2 : 4;
  if( slot < 0 || slot >= (int) c->slots.size() || !c->slots[slot].p[0] ) return outRefuse( c, "no such slot", who );
  if( method > VVR_HASH_CHECKSUM ) return outRefuse( c, "unknown method", who );
  if( rq->job < -1 ) return outRefuse( c, "job must be a job id or -1", who );
  if( !rq->digest && !rq->expected ) return outRefuse( c, "neither digest nor expected given", who );
  if( rq->expected && !rq->mismatch ) return outRefuse( c, "expected without mismatch", who );
  const bool two = c->cfg.bit_depth > 8;
  const DevPlanes d = pictureIn( c, slot );      // (the picture in the slot, not the slot)
  hipSetDevice( c->device );
  // ---- 2. a ring entry; the picture has been handed to the device
  OutEntry* e = nullptr;
  hipEvent_t jobDone = nullptr; int jobFailed = VVR_OK;
  std::unique_lock<std::mutex> lk( c->mu );
  { const int rc = outAcquire( c, who, slot, rq->job, rq->blocking != 0, lk, e, jobDone, jobFailed ); if( rc != VVR_OK ) return rc; }
  hipStream_t s = c->outQStream;
  outTake( c, e, slot, rq->job, jobFailed );
  e->hash = method + 1; e->hashNc = nc; e->digest = rq->digest; e->mismatch = rq->mismatch; e->verify = rq->expected != nullptr;
  if( rq->expected ) memcpy( e->expected, rq->expected, (size_t) nc * len );
  if( jobFailed != VVR_OK ) { e->state = OQ_FLIGHT; return e->ticket; }      // (nothing to run: the request fails with the job's status)
  // ---- the entry's buffers.  MD5: the planes' bytes, on the device and pinned; else a word per row on the device, a word per component on both sides
  size_t total = 0, rowsTotal = 0; double planesBytes = 0;
  for( int k = 0; k < nc; k++ )
  {
    e->off[k] = total; e->planeBytes[k] = (size_t) d.w[k] * d.h[k] * ( two ? 2 : 1 );
    total += alignUp( e->planeBytes[k], 256 ); rowsTotal += d.h[k]; planesBytes += (double) d.w[k] * d.h[k] * sizeof( pel_t );
  }
  const size_t wordsOff = alignUp( sizeof( uint32_t ) * rowsTotal, 256 );
  if( outGrow( e->dev, e->devCap, method == VVR_HASH_MD5 ? total : wordsOff + 256, false ) != VVR_OK || outGrow( e->host, e->hostCap, method == VVR_HASH_MD5 ? total : 256, true ) != VVR_OK )
  { c->setError( std::string( who ) + ": out of device or pinned memory" ); return VVR_ERR_DEVICE; }
  // ---- 3. behind the picture (or the slot's users) on the device, 4. the kernels.  mu stays held up to the registration of the `read` event (as vvr_output_submit)
  OQCHK( outOrder( c, e, slot, rq->job, jobDone ) );
  if( method == VVR_HASH_MD5 )
    for( int k = 0; k < nc; k++ ) launch_output_window( s, d.p[k], d.stride[k], d.w[k], d.h[k], two ? 2 : 1, e->dev + e->off[k] );
  else
  {
    const HashParams p = hash_params( d, nc, two, method == VVR_HASH_CRC );
    outTimeBegin( c, s, e->timed, e->timing, K_HASH_ROWS, planesBytes + sizeof( uint32_t ) * rowsTotal );
    launch_hash_rows( s, p, (uint32_t*) e->dev );
    if( e->timed ) hipEventRecord( e->timing.b, s );
    outTimeBegin( c, s, e->timed2, e->timing2, K_HASH_COMBINE, (double) sizeof( uint32_t ) * ( rowsTotal + nc ) );
    launch_hash_combine( s, p, (const uint32_t*) e->dev, (uint32_t*) ( e->dev + wordsOff ) );
    if( e->timed2 ) hipEventRecord( e->timing2.b, s );
  }
  OQCHK( hipGetLastError() );
  OQCHK( hipEventRecord( e->read, s ) );
  c->slotExt[slot].push_back( e->read );
  e->state = OQ_FLIGHT; e->queued = true;
  const int ticket = e->ticket;
  lk.unlock();
  // ---- the result's way to the host: nc words, or the planes' bytes
  hipError_t ce = hipSuccess;
  if( method != VVR_HASH_MD5 ) ce = hipMemcpyAsync( e->host, e->dev + wordsOff, sizeof( uint32_t ) * nc, hipMemcpyDeviceToHost, s );
  else for( int k = 0; k < nc && ce == hipSuccess; k++ ) ce = hipMemcpyAsync( e->host + e->off[k], e->dev + e->off[k], e->planeBytes[k], hipMemcpyDeviceToHost, s );
  if( ce == hipSuccess ) ce = hipEventRecord( e->done, s );
  if( ce != hipSuccess )
  {
    hipStreamSynchronize( s );
    lk.lock(); e->rc = VVR_ERR_DEVICE; e->queued = false; c->setError( std::string( who ) + ": copy to the host: " + hipGetErrorString( ce ) );
  }
  return ticket;
}

VVR_API int vvr_stats_submit( vvr_context* c, const vvr_stats_request* rq )
{
  if( !c || !rq ) return VVR_ERR_PARAMETER;
  const char* const who = "vvr_stats_submit";
  // ---- 1. the request
  if( rq->struct_size != sizeof( vvr_stats_request ) ) return outRefuse( c, "struct_size is not sizeof( vvr_stats_request )", who );
  const int slot = rq->slot, bd = c->cfg.bit_depth, nc = c->cfg.chroma_format ? 3 : 1, x = rq->x, y = rq->y, w = rq->w, h = rq->h;
  if( slot < 0 || slot >= (int) c->slots.size() || !c->slots[slot].p[0] ) return outRefuse( c, "no such slot", who );
  if( rq->job < -1 ) return outRefuse( c, "job must be a job id or -1", who );
  if( rq->mode > VVR_STATS_RGB ) return outRefuse( c, "unknown mode", who );
  if( !rq->stats ) return outRefuse( c, "stats is NULL", who );
  const bool rgb = rq->mode == VVR_STATS_RGB;
  int outMatrix = 0, outFullRange = 0;      // (looked at here for the refusal, taken under mu where the request is accepted: as vvr_output_submit)
  if( rgb )
  {
    { std::lock_guard<std::mutex> lk( c->mu ); outMatrix = c->outMatrix; }
    if( nc == 1 ) return outRefuse( c, "RGB statistics of a 4:0:0 context: there is no chroma to convert", who );
    if( !outMatrix ) return outRefuse( c, "RGB statistics with no colour description set (vvr_set_output_colour)", who );
  }
  const DevPlanes d = pictureIn( c, slot );      // (the picture in the slot, not the slot)
  if( x < 0 || y < 0 || w <= 0 || h <= 0 || x + w > d.w[0] || y + h > d.h[0] || ( nc > 1 && ( ( x | y | w | h ) & 1 ) ) ) return outRefuse( c, "window outside the picture, empty, or odd in 4:2:0", who );
  hipSetDevice( c->device );
  // ---- 2. a ring entry; the picture has been handed to the device
  OutEntry* e = nullptr;
  hipEvent_t jobDone = nullptr; int jobFailed = VVR_OK;
  std::unique_lock<std::mutex> lk( c->mu );
  { const int rc = outAcquire( c, who, slot, rq->job, rq->blocking != 0, lk, e, jobDone, jobFailed ); if( rc != VVR_OK ) return rc; }
  hipStream_t s = c->outQStream;
  if( rgb ) { outMatrix = c->outMatrix; outFullRange = c->outFullRange; }      // (what is set now, behind the waits above)
  outTake( c, e, slot, rq->job, jobFailed );
  e->stats = rq->mode + 1; e->statsW = w; e->statsH = h; e->statsOut = rq->stats;
  if( jobFailed != VVR_OK ) { e->state = OQ_FLIGHT; return e->ticket; }      // (nothing to run: the request fails with the job's status)
  // ---- the entry's buffers: the copies of the words the workgroups add into, the folded words behind them; the folded words pinned
  const size_t shardBytes = alignUp( sizeof( uint32_t ) * STATS_SHARDS * STATS_WORDS, 256 ), wordBytes = sizeof( uint32_t ) * STATS_WORDS;
  if( outGrow( e->dev, e->devCap, shardBytes + wordBytes, false ) != VVR_OK || outGrow( e->host, e->hostCap, wordBytes, true ) != VVR_OK )
  { c->setError( std::string( who ) + ": out of device or pinned memory" ); return VVR_ERR_DEVICE; }
  // ---- 3. behind the picture (or the slot's users) on the device, 4. the clear and the kernels.  mu stays held up to the registration of the `read` event (as vvr_output_submit)
  OQCHK( outOrder( c, e, slot, rq->job, jobDone ) );
  OQCHK( hipMemsetAsync( e->dev, 0, shardBytes, s ) );
  OutputRgbParams p; memset( &p, 0, sizeof( p ) );
  for( int k = 0; k < nc; k++ ) { const int sh = k ? 1 : 0; p.src[k] = d.p[k] + (size_t) ( y >> sh ) * d.stride[k] + ( x >> sh ); p.stride[k] = d.stride[k]; }
  p.w = w; p.h = h; p.collocated = rq->collocated & 3; p.format = RGB_FMT_STATS; p.maxVal = ( 1 << bd ) - 1;
  if( rgb ) rgb_coefficients( outMatrix, outFullRange, bd, bd, p );      // (od = bd: the input of the transform stage)
  outTimeBegin( c, s, e->timed, e->timing, K_OUTPUT_STATS, (double) w * h * ( rgb ? 3. : 2. ) );      // (read: 2 bytes of luma, 2 x 2 / 4 of chroma)
  launch_output_stats( s, p, rgb ? 1 : 0, (uint32_t*) e->dev );
  if( e->timed ) hipEventRecord( e->timing.b, s );
  OQCHK( hipGetLastError() );
  OQCHK( hipEventRecord( e->read, s ) );      // (the slot's reader ends here: the fold reads the entry's scratch)
  c->slotExt[slot].push_back( e->read );
  e->state = OQ_FLIGHT; e->queued = true;
  outTimeBegin( c, s, e->timed2, e->timing2, K_OUTPUT_STATS_SUM, (double) wordBytes * ( STATS_SHARDS + 1 ) );
  launch_output_stats_sum( s, (const uint32_t*) e->dev, (uint32_t*) ( e->dev + shardBytes ) );
  if( e->timed2 ) hipEventRecord( e->timing2.b, s );
  const int ticket = e->ticket;
  lk.unlock();
  // ---- the result's way to the host: the words
  hipError_t ce = hipGetLastError();
  if( ce == hipSuccess ) ce = hipMemcpyAsync( e->host, e->dev + shardBytes, wordBytes, hipMemcpyDeviceToHost, s );
  if( ce == hipSuccess ) ce = hipEventRecord( e->done, s );
  if( ce != hipSuccess )
  {
    hipStreamSynchronize( s );
    lk.lock(); e->rc = VVR_ERR_DEVICE; e->queued = false; c->setError( std::string( who ) + ": copy to the host: " + hipGetErrorString( ce ) );
  }
  return ticket;
}

// vvr_compare_submit and vvr_ssim_submit (`who`): one path for the window, the reference's home and staging, the ring entry, the ordering behind
// both slots and the result's way back; `ssim` selects the refusal of windows below 8 x 8, the size of a record, the kernels and what
// vvr_output_wait writes.  A vvr_ssim_request is a vvr_compare_request field by field (result and map are pointers to other types)
static_assert( sizeof( vvr_ssim_request ) == sizeof( vvr_compare_request ) && offsetof( vvr_ssim_request, ref ) == offsetof( vvr_compare_request, ref ) &&
               offsetof( vvr_ssim_request, result ) == offsetof( vvr_compare_request, result ) && offsetof( vvr_ssim_request, map ) == offsetof( vvr_compare_request, map ), "vvr_ssim_request mirrors vvr_compare_request" );
static int compareSubmit( vvr_context* c, const vvr_compare_request* rq, const char* who, bool ssim, int scales = 0, const XpsnrAsk* xp = nullptr )      // scales > 0: vvr_msssim_submit; xp: vvr_xpsnr_submit
{
  const bool ms = scales > 0;
  const int temporal = xp ? xp->temporal : 0;
  // ---- 1. the request (its struct_size has been looked at)
  const int slot = rq->slot, refSlot = rq->ref_slot, nc = c->cfg.chroma_format ? 3 : 1, x = rq->x, y = rq->y, winW = rq->w, winH = rq->h;
  // the scaling the request takes (vvr_set_compare_scaling): the one that is set now, whatever is set while the request is in flight
  int scaleW = 0, scaleH = 0, scaleCol = 0;
  { std::lock_guard<std::mutex> g( c->mu ); scaleW = c->cmpScaleW; scaleH = c->cmpScaleH; scaleCol = c->cmpScaleCollocated; }
  const bool scaled = scaleW != 0;
  if( slot < 0 || slot >= (int) c->slots.size() || !c->slots[slot].p[0] ) return outRefuse( c, "no such slot", who );
  if( refSlot < -1 || refSlot >= (int) c->slots.size() || ( refSlot >= 0 && !c->slots[refSlot].p[0] ) ) return outRefuse( c, "no such ref_slot", who );
  if( refSlot == slot ) return outRefuse( c, "ref_slot is the slot itself", who );
  if( rq->job < -1 ) return outRefuse( c, "job must be a job id or -1", who );
  if( !rq->result ) return outRefuse( c, "result is NULL", who );
  const DevPlanes d = pictureIn( c, slot );      // (the picture in the slot, not the slot)
  if( x < 0 || y < 0 || winW <= 0 || winH <= 0 || x + winW > d.w[0] || y + winH > d.h[0] || ( nc > 1 && ( ( x | y | winW | winH ) & 1 ) ) ) return outRefuse( c, "window outside the picture, empty, or odd in 4:2:0", who );
  if( scaled && refSlot >= 0 ) return outRefuse( c, "ref_slot while vvr_set_compare_scaling is on (two slots of different picture sizes are not offered)", who );
  if( scaled && ( winW > 8 * scaleW || scaleW > 8 * winW || winH > 8 * scaleH || scaleH > 8 * winH ) ) return outRefuse( c, "the size of vvr_set_compare_scaling is not within 1/8 .. 8 times the window's", who );
  // w x h: what is measured - the window, or the window rescaled; everything from here on but the window's origin in the slot takes it
  const int w = scaled ? scaleW : winW, h = scaled ? scaleH : winH;
  if( ssim && ( w < 8 || h < 8 ) ) return outRefuse( c, "a window below 8 x 8 holds no SSIM window", who );
  uint32_t xpB = 0, xpBx = 0, xpBy = 0;
  if( xp && ( w < 8 || h < 8 ) ) return outRefuse( c, "a window below 8 x 8", who );
  if( xp && vvr_xpsnr_blocks( w, h, xp->block, &xpB, &xpBx, &xpBy ) != VVR_OK ) return outRefuse( c, "more than 16384 blocks", who );
  for( int k = 0; k < nc && ms; k++ )
    if( ( ( w >> ( k ? 1 : 0 ) ) >> ( scales - 1 ) ) < 8 || ( ( h >> ( k ? 1 : 0 ) ) >> ( scales - 1 ) ) < 8 ) return outRefuse( c, "a component has no 8 x 8 window at the last level: the window takes fewer scales", who );
  const int rb = refSlot >= 0 ? 2 : rq->ref_bytes_per_sample;
  CompareParams p; memset( &p, 0, sizeof( p ) );
  size_t rowBytes[3] = { 0, 0, 0 }, extent[3] = { 0, 0, 0 };
  size_t prevExtent[2] = { 0, 0 };
  for( int k = 0; k < nc; k++ ) { const int sh = k ? 1 : 0; p.w[k] = w >> sh; p.h[k] = h >> sh; p.src[k] = d.p[k] + (size_t) ( y >> sh ) * d.stride[k] + ( x >> sh ); p.stride[k] = d.stride[k]; }
  p.numComp = nc; p.refBytes = rb; p.nbx = ( w + 63 ) / 64; p.nby = ( h + 63 ) / 64;
  if( refSlot >= 0 )
  {
    const DevPlanes r = pictureIn( c, refSlot );
    if( r.w[0] != d.w[0] || r.h[0] != d.h[0] ) return outRefuse( c, "the pictures in slot and ref_slot are of different sizes", who );
    for( int k = 0; k < nc; k++ ) { const int sh = k ? 1 : 0; p.ref[k] = (const uint8_t*) ( r.p[k] + (size_t) ( y >> sh ) * r.stride[k] + ( x >> sh ) ); p.refStride[k] = (size_t) r.stride[k] * sizeof( pel_t ); }
  }
  else
  {
    if( rb != 1 && rb != 2 ) return outRefuse( c, "ref_bytes_per_sample must be 1 or 2", who );
    for( int k = 0; k < nc; k++ )
    {
      rowBytes[k] = (size_t) p.w[k] * rb; extent[k] = (size_t) ( p.h[k] - 1 ) * rq->ref_stride_bytes[k] + rowBytes[k];
      if( !rq->ref[k] || rq->ref_stride_bytes[k] < rowBytes[k] ) return outRefuse( c, "missing reference plane or stride below the window's row", who );
    }
  }
  if( temporal && rb != 1 && rb != 2 ) return outRefuse( c, "ref_bytes_per_sample must be 1 or 2", who );
  const size_t prevRow = (size_t) w * rb;      // (the prev planes of an XPSNR request: luma of the window's size, always the caller's memory)
  for( int k = 0; k < temporal; k++ )
  {
    if( !xp->prev[k] || xp->prevStride[k] < prevRow ) return outRefuse( c, "missing prev plane or stride below the window's row", who );
    prevExtent[k] = (size_t) ( h - 1 ) * xp->prevStride[k] + prevRow;
  }
  hipSetDevice( c->device );
  std::unique_lock<std::mutex> lk( c->mu );
  // ---- where the reference lies: device memory the context knows (every plane wholly inside a range), or the host
  int devPlanes = 0;
  for( int k = 0; k < nc && refSlot < 0; k++ )
  {
    const char* b = (const char*) rq->ref[k];
    for( const DevRange& r : c->devRanges )
    {
      if( b >= r.p && b + extent[k] <= r.p + r.n ) { devPlanes++; break; }
      if( b < r.p + r.n && b + extent[k] > r.p ) { c->setError( std::string( who ) + ": a reference plane lies partly inside a device range (vvr_device_alloc / vvr_device_register)" ); return VVR_ERR_PARAMETER; }
    }
  }
  for( int k = 0; k < temporal; k++ )
  {
    const char* b = (const char*) xp->prev[k];
    for( const DevRange& r : c->devRanges )
    {
      if( b >= r.p && b + prevExtent[k] <= r.p + r.n ) { devPlanes++; break; }
      if( b < r.p + r.n && b + prevExtent[k] > r.p ) { c->setError( std::string( who ) + ": a prev plane lies partly inside a device range (vvr_device_alloc / vvr_device_register)" ); return VVR_ERR_PARAMETER; }
    }
  }
  if( devPlanes && devPlanes != ( refSlot < 0 ? nc : 0 ) + temporal ) { c->setError( std::string( who ) + ": reference planes in device memory mixed with planes in host memory" ); return VVR_ERR_PARAMETER; }
  // (staged: the reference planes go through `tmp`; stagedPrev: the prev planes of an XPSNR request do, behind them - also beside a ref_slot)
  const bool devRef = devPlanes != 0, staged = refSlot < 0 && !devRef, stagedPrev = temporal && !devRef;
  bool pinnedRef = staged || stagedPrev;
  for( int k = 0; k < nc && pinnedRef && staged; k++ ) pinnedRef = c->pinned.contains( rq->ref[k], extent[k] );
  for( int k = 0; k < temporal && pinnedRef; k++ ) pinnedRef = c->pinned.contains( xp->prev[k], prevExtent[k] );
  // ---- the entry's buffers: the blocks' records, the folded words and the map behind them; a reference from the host packed in `tmp`, rows at a
  // multiple of 16 bytes; pinned: the folded words and the map, then the staging of a reference in pageable memory
  const int blocks = p.nbx * p.nby, recWords = ssim ? SSIM_REC_WORDS : CMP_REC_WORDS, outWords = ssim ? SSIM_OUT_WORDS : CMP_OUT_WORDS;
  size_t recBytes = alignUp( sizeof( uint32_t ) * recWords * nc * blocks, 256 ), wordBytes = sizeof( uint32_t ) * ( CMP_HEAD_WORDS + blocks );
  size_t crossBytes = sizeof( uint32_t ) * ( rq->map ? CMP_HEAD_WORDS + blocks : 3 * outWords );
  // MS-SSIM: the records of every level one after the other, each at a multiple of 256 bytes, the words of all levels, then the pyramid - per level
  // k >= 1 and component the slot's side and the reference's, 16-bit words, rows a multiple of 16 bytes, each plane at a multiple of 256 bytes
  MsssimFold fold; memset( &fold, 0, sizeof( fold ) );
  size_t pyrOff[MSSSIM_MAX_SCALES][3][2]; int pyrStride[MSSSIM_MAX_SCALES][3]; size_t pyrBytes = 0;
  if( ms )
  {
    fold.scales = scales; recBytes = 0;
    for( int k = 0; k < scales; k++ )
    {
      fold.recOff[k] = (int) ( recBytes / sizeof( uint32_t ) ); fold.blocks[k] = ( ( ( w >> k ) + 63 ) / 64 ) * ( ( ( h >> k ) + 63 ) / 64 );
      recBytes += alignUp( sizeof( uint32_t ) * MSSSIM_REC_WORDS * nc * fold.blocks[k], 256 );
      for( int q = 0; q < nc && k > 0; q++ )
      {
        pyrStride[k][q] = (int) alignUp( (size_t) ( p.w[q] >> k ), 8 );
        for( int side = 0; side < 2; side++ ) { pyrOff[k][q][side] = pyrBytes; pyrBytes += alignUp( sizeof( uint16_t ) * pyrStride[k][q] * ( p.h[q] >> k ), 256 ); }
      }
    }
    wordBytes = sizeof( uint32_t ) * MSSSIM_OUT_WORDS * 3 * MSSSIM_MAX_SCALES; crossBytes = sizeof( uint32_t ) * MSSSIM_OUT_WORDS * nc * scales;
  }
  // XPSNR: the records are the words - cleared on the device, added to by the one launch, copied back whole
  if( xp ) { recBytes = 0; wordBytes = crossBytes = sizeof( unsigned long long ) * XPSNR_REC_WORDS * xpBx * xpBy; }
  const size_t hostStageOff = alignUp( wordBytes, 256 ), pyrBase = alignUp( recBytes + wordBytes, 256 );
  // the rescaled window (vvr_set_compare_scaling): behind all of that, 16-bit planes as k_rescale stores them - rows back to back - each at a
  // multiple of 256 bytes.  Not for a comparison: k_output_compare_scaled rescales and compares in one pass (`fused`)
  const bool fused = scaled && !ssim && !ms && !xp;
  const size_t scaleBase = alignUp( ms ? pyrBase + pyrBytes : recBytes + wordBytes, 256 );
  size_t scaleOff[3] = { 0, 0, 0 }, scaleBytes = 0;
  for( int k = 0; k < nc && scaled && !fused; k++ ) { scaleOff[k] = scaleBytes; scaleBytes += alignUp( sizeof( uint16_t ) * p.w[k] * p.h[k], 256 ); }
  size_t stageOff[3] = { 0, 0, 0 }, stageStride[3] = { 0, 0, 0 }, stageBytes = 0;
  for( int k = 0; k < nc && staged; k++ ) { stageOff[k] = stageBytes; stageStride[k] = alignUp( rowBytes[k], 16 ); stageBytes += alignUp( stageStride[k] * p.h[k], 256 ); }
  size_t prevStageOff[2] = { 0, 0 }; const size_t prevStageStride = alignUp( prevRow, 16 );
  for( int k = 0; k < temporal && stagedPrev; k++ ) { prevStageOff[k] = stageBytes; stageBytes += alignUp( prevStageStride * h, 256 ); }
  // ---- a reference in pageable memory goes into an entry's pinned memory BEFORE the request is ordered: from outAcquire to the registration of the
  // `read` event mu stays held (a picture committed in between that overwrites the slot has to find the event), and a frame's worth of memcpy
  // does not belong under mu.  The entry is this thread's meanwhile and is handed to outAcquire as the one to take
  OutEntry* mine = nullptr;
  if( ( staged || stagedPrev ) && !pinnedRef )
  {
    if( !c->outRing ) c->outRing = new OutEntry[VVR_OUT_RING];
    for( int i = 0; i < VVR_OUT_RING && !mine; i++ ) if( c->outRing[i].state == OQ_FREE ) mine = &c->outRing[i];
    if( !mine ) { c->setError( std::string( who ) + ": 8 requests in flight (vvr_output_wait retires one)" ); return VVR_ERR_BUSY; }
    if( outGrow( mine->host, mine->hostCap, hostStageOff + stageBytes, true ) != VVR_OK ) { c->setError( std::string( who ) + ": out of device or pinned memory" ); return VVR_ERR_DEVICE; }
    mine->state = OQ_WAITING; mine->ticket = -1; mine->devDst = false;
    lk.unlock();
    for( int k = 0; k < nc && staged; k++ )
      for( int r = 0; r < p.h[k]; r++ ) memcpy( mine->host + hostStageOff + stageOff[k] + (size_t) r * stageStride[k], (const char*) rq->ref[k] + (size_t) r * rq->ref_stride_bytes[k], rowBytes[k] );
    for( int k = 0; k < temporal; k++ )
      for( int r = 0; r < h; r++ ) memcpy( mine->host + hostStageOff + prevStageOff[k] + (size_t) r * prevStageStride, (const char*) xp->prev[k] + (size_t) r * xp->prevStride[k], prevRow );
    lk.lock();
    mine->state = OQ_FREE;
  }
  // ---- 2. a ring entry; the picture has been handed to the device - and with ref_slot every picture: who uses that slot is only known then
  if( refSlot >= 0 && !c->bySeq.empty() )
  {
    if( !rq->blocking ) return VVR_NOT_READY;
    c->cv.wait( lk, [&]{ return c->bySeq.empty(); } );
  }
  OutEntry* e = nullptr;
  hipEvent_t jobDone = nullptr; int jobFailed = VVR_OK;
  { const int rc = outAcquire( c, who, slot, rq->job, rq->blocking != 0, lk, e, jobDone, jobFailed, mine ); if( rc != VVR_OK ) return rc; }
  hipStream_t s = c->outQStream;
  outTake( c, e, slot, rq->job, jobFailed );
  e->cmp = nc; e->cmpW = w; e->cmpH = h; e->cmpBlocks = blocks; e->cmpOut = rq->result; e->cmpMap = rq->map; e->cmpSsim = ssim; e->msScales = scales;
  if( xp ) { e->xps = true; e->xpsTemporal = temporal; e->xpsFilter = xp->filter ? xp->filter : ( (int64_t) w * h > 2048 * 1152 ? 2 : 1 ); e->xpsBlock = (int) xpB; e->xpsBx = (int) xpBx; e->xpsBy = (int) xpBy; e->xpsBlocks = xp->blocks; }
  if( jobFailed != VVR_OK ) { e->state = OQ_FLIGHT; return e->ticket; }      // (nothing to run: the request fails with the job's status)
  if( outGrow( e->dev, e->devCap, scaleBase + scaleBytes, false ) != VVR_OK || outGrow( e->tmp, e->tmpCap, stageBytes, false ) != VVR_OK ||
      outGrow( e->host, e->hostCap, hostStageOff, true ) != VVR_OK )      // (a staged reference: grown above, beyond this)
  { c->setError( std::string( who ) + ": out of device or pinned memory" ); return VVR_ERR_DEVICE; }
  for( int k = 0; k < nc && refSlot < 0; k++ )
  {
    p.ref[k] = staged ? (const uint8_t*) ( e->tmp + stageOff[k] ) : (const uint8_t*) rq->ref[k];
    p.refStride[k] = staged ? stageStride[k] : rq->ref_stride_bytes[k];
  }
  // wide loads (vvr_device.h): not from an odd origin of a 4:0:0 window, not from reference planes whose base or stride is odd
  p.bySample = nc == 1 && ( x & 1 );
  // the rescaled window: k_rescale reads the slot, the measure reads the entry's planes, whose rows lie back to back - a plane of odd width is not
  // one for wide loads
  RescaleParams rs[3];
  for( int k = 0; k < nc && scaled; k++ )
  {
    // (as vvr_read_output_scaled: the component's subsampling, luma always collocated)
    const bool luma = k == 0;
    const int cs = luma ? 0 : 1, colX = luma ? 1 : scaleCol & 1, colY = luma ? 1 : ( scaleCol >> 1 ) & 1, fracShift = luma ? 4 : 5;
    RescaleParams& r = rs[k];
    r.src = p.src[k]; r.stride = p.stride[k]; r.w = winW >> cs; r.h = winH >> cs; r.outW = p.w[k]; r.outH = p.h[k];
    r.luma = luma; r.maxVal = ( 1 << c->cfg.bit_depth ) - 1; r.bytesPerSample = 2;
    int scale;
    rescale_axis( r.w, r.outW, cs, colX, fracShift, scale, r.addX, r.shiftX ); r.stepX = scale << cs;
    rescale_axis( r.h, r.outH, cs, colY, fracShift, scale, r.addY, r.shiftY ); r.stepY = scale << cs;
    if( k == 0 ) p.bySample = 0;
    if( fused ) continue;      // (k_output_compare_scaled reads the slot itself, sample by sample)
    p.src[k] = (const pel_t*) ( e->dev + scaleBase + scaleOff[k] ); p.stride[k] = p.w[k];
    if( p.w[k] & 1 ) p.bySample = 1;
  }
  for( int k = 0; k < nc; k++ ) if(( (uintptr_t) p.ref[k] | p.refStride[k] ) & 1 ) p.bySample = 1;
  XpsnrParams xq; memset( &xq, 0, sizeof( xq ) );
  for( int k = 0; k < temporal; k++ )
  {
    xq.prev[k] = stagedPrev ? (const uint8_t*) ( e->tmp + prevStageOff[k] ) : (const uint8_t*) xp->prev[k];
    xq.prevStride[k] = stagedPrev ? prevStageStride : xp->prevStride[k];
    if( ( (uintptr_t) xq.prev[k] | xq.prevStride[k] ) & 1 ) p.bySample = 1;
  }
  if( devRef )      // (vvr_device_free / vvr_device_unregister see a request in flight that uses the range)
  {
    e->direct = true; e->devDst = true; e->nc = 0;
    for( int k = 0; k < nc && refSlot < 0; k++ ) { e->dst[e->nc] = const_cast<void*>( rq->ref[k] ); e->extent[e->nc++] = extent[k]; }
    for( int k = 0; k < temporal; k++ ) { e->dst[e->nc] = const_cast<void*>( xp->prev[k] ); e->extent[e->nc++] = prevExtent[k]; }
  }
  // ---- 3. behind the picture (or the slot's users) and behind all that uses ref_slot on the device, 4. the reference's copy and the kernels.
  // mu stays held up to the registration of the `read` event (as vvr_output_submit)
  OQCHK( outOrder( c, e, slot, rq->job, jobDone ) );
  if( refSlot >= 0 ) OQCHK( outOrder( c, e, refSlot, -1, nullptr ) );
  if( scaled && !fused )      // (the slot's last reader: the `read` event is recorded behind it, the measure reads the entry's planes)
  {
    double rsBytes = 0;
    for( int k = 0; k < nc; k++ ) rsBytes += sizeof( pel_t ) * ( (double) rs[k].w * rs[k].h + (double) rs[k].outW * rs[k].outH );
    outTimeBegin( c, s, e->timed0, e->timing0, K_COMPARE_RESCALE, rsBytes );
    for( int k = 0; k < nc; k++ ) launch_rescale( s, rs[k], e->dev + scaleBase + scaleOff[k] );
    if( e->timed0 ) hipEventRecord( e->timing0.b, s );
    e->rescales = nc;
    OQCHK( hipGetLastError() );
    OQCHK( hipEventRecord( e->read, s ) );
  }
  if( ( staged || stagedPrev ) && !pinnedRef ) OQCHK( hipMemcpyAsync( e->tmp, e->host + hostStageOff, stageBytes, hipMemcpyHostToDevice, s ) );
  for( int k = 0; k < nc && staged && pinnedRef; k++ )
    OQCHK( hipMemcpy2DAsync( e->tmp + stageOff[k], stageStride[k], rq->ref[k], rq->ref_stride_bytes[k], rowBytes[k], p.h[k], hipMemcpyHostToDevice, s ) );
  for( int k = 0; k < temporal && stagedPrev && pinnedRef; k++ )
    OQCHK( hipMemcpy2DAsync( e->tmp + prevStageOff[k], prevStageStride, xp->prev[k], xp->prevStride[k], prevRow, h, hipMemcpyHostToDevice, s ) );
  uint32_t* recs = (uint32_t*) e->dev; uint32_t* words = (uint32_t*) ( e->dev + recBytes );
  double samples = 0;
  for( int k = 0; k < nc; k++ ) samples += (double) p.w[k] * p.h[k];
  // (MS-SSIM: level k reads 2 + rb or 4 bytes a sample and, but for the last, writes 4 bytes for every four samples; level l holds samples / 4^l)
  auto level = [&]( int k, MsssimNext& nx )      // the planes of level k >= 1 of the pyramid
  {
    for( int q = 0; q < nc; q++ ) { nx.x[q] = (uint16_t*) ( e->dev + pyrBase + pyrOff[k][q][0] ); nx.y[q] = (uint16_t*) ( e->dev + pyrBase + pyrOff[k][q][1] ); nx.stride[q] = pyrStride[k][q]; }
  };
  double msBytes = 0;
  for( int k = 0; k < scales; k++ ) msBytes += samples / (double) ( 1 << 2 * k ) * ( ( k ? 4 : 2 + rb ) + ( k + 1 < scales ? 1 : 0 ) );
  if( xp ) OQCHK( hipMemsetAsync( e->dev, 0, wordBytes, s ) );      // (the records k_output_xpsnr adds to)
  double fusedBytes = samples * rb;      // (read: the window in the slot and the reference)
  for( int k = 0; k < nc && fused; k++ ) fusedBytes += sizeof( pel_t ) * (double) rs[k].w * rs[k].h;
  outTimeBegin( c, s, e->timed, e->timing, fused ? K_OUTPUT_COMPARE_SCALED : xp ? K_OUTPUT_XPSNR : ms ? K_OUTPUT_MSSSIM : ssim ? K_OUTPUT_SSIM : K_OUTPUT_COMPARE,
                fused ? fusedBytes : ms ? msBytes : samples * ( 2 + rb ) + (double) temporal * w * h * rb );
  MsssimNext nx; memset( &nx, 0, sizeof( nx ) );
  if( xp )
  {
    xq.c = p; xq.block = e->xpsBlock; xq.blocksX = e->xpsBx; xq.blocksY = e->xpsBy; xq.filter = e->xpsFilter; xq.temporal = temporal;
    launch_output_xpsnr( s, xq, (unsigned long long*) e->dev );
  }
  else if( ms ) { if( scales > 1 ) level( 1, nx ); launch_output_msssim( s, p, c->cfg.bit_depth, recs, scales > 1 ? &nx : nullptr ); }
  else if( ssim ) launch_output_ssim( s, p, c->cfg.bit_depth, recs, (int32_t*) ( words + CMP_HEAD_WORDS ) );
  else if( fused )
  {
    CompareScaledParams sp; memset( &sp, 0, sizeof( sp ) );
    for( int k = 0; k < nc; k++ ) { sp.rs[k] = rs[k]; sp.ref[k] = p.ref[k]; sp.refStride[k] = p.refStride[k]; }
    sp.numComp = nc; sp.refBytes = rb; sp.nbx = p.nbx; sp.nby = p.nby; sp.byByte = p.bySample;
    launch_output_compare_scaled( s, sp, recs, words + CMP_HEAD_WORDS );
  }
  else launch_output_compare( s, p, recs, words + CMP_HEAD_WORDS );
  if( e->timed && scales <= 1 ) hipEventRecord( e->timing.b, s );
  OQCHK( hipGetLastError() );
  if( !scaled || fused ) OQCHK( hipEventRecord( e->read, s ) );      // (the slots' reader ends here: the fold reads the entry's scratch)
  c->slotExt[slot].push_back( e->read );
  if( refSlot >= 0 ) { c->slotExt[refSlot].push_back( e->read ); e->refSlot = refSlot; }
  e->state = OQ_FLIGHT; e->queued = true;
  for( int k = 1; k < scales; k++ )      // the deeper levels of an MS-SSIM request: both images from the pyramid, the wide class
  {
    CompareParams q = p; MsssimNext from; memset( &from, 0, sizeof( from ) );
    level( k, from );
    for( int n = 0; n < nc; n++ ) { q.w[n] = p.w[n] >> k; q.h[n] = p.h[n] >> k; q.src[n] = (const pel_t*) from.x[n]; q.stride[n] = from.stride[n]; q.ref[n] = (const uint8_t*) from.y[n]; q.refStride[n] = sizeof( uint16_t ) * from.stride[n]; }
    q.refBytes = 2; q.bySample = 0; q.nbx = ( q.w[0] + 63 ) / 64; q.nby = ( q.h[0] + 63 ) / 64;
    if( k + 1 < scales ) level( k + 1, nx );
    launch_output_msssim( s, q, c->cfg.bit_depth, recs + fold.recOff[k], k + 1 < scales ? &nx : nullptr );
    if( e->timed && k + 1 == scales ) hipEventRecord( e->timing.b, s );
  }
  if( !xp )      // (an XPSNR request has no fold: its blocks are summed on the host)
  {
    outTimeBegin( c, s, e->timed2, e->timing2, ms ? K_OUTPUT_MSSSIM_SUM : ssim ? K_OUTPUT_SSIM_SUM : K_OUTPUT_COMPARE_SUM, ms ? (double) recBytes + crossBytes : (double) sizeof( uint32_t ) * ( recWords * blocks + outWords ) * nc );
    if( ms ) launch_output_msssim_sum( s, recs, fold, nc, words );
    else if( ssim ) launch_output_ssim_sum( s, recs, blocks, nc, words );
    else launch_output_compare_sum( s, recs, blocks, nc, words );
  }
  if( e->timed2 ) hipEventRecord( e->timing2.b, s );
  const int ticket = e->ticket;
  lk.unlock();
  // ---- the result's way to the host: the folded words, with `map` a word per block behind them
  hipError_t ce = hipGetLastError();
  if( ce == hipSuccess ) ce = hipMemcpyAsync( e->host, words, crossBytes, hipMemcpyDeviceToHost, s );
  if( ce == hipSuccess ) ce = hipEventRecord( e->done, s );
  if( ce != hipSuccess )
  {
    hipStreamSynchronize( s );
    lk.lock(); e->rc = VVR_ERR_DEVICE; e->queued = false; c->setError( std::string( who ) + ": copy to the host: " + hipGetErrorString( ce ) );
  }
  return ticket;
}
VVR_API int vvr_compare_submit( vvr_context* c, const vvr_compare_request* rq )
{
  if( !c || !rq ) return VVR_ERR_PARAMETER;
  if( rq->struct_size != sizeof( vvr_compare_request ) ) return outRefuse( c, "struct_size is not sizeof( vvr_compare_request )", "vvr_compare_submit" );
  return compareSubmit( c, rq, "vvr_compare_submit", false );
}
VVR_API int vvr_ssim_submit( vvr_context* c, const vvr_ssim_request* rq )
{
  if( !c || !rq ) return VVR_ERR_PARAMETER;
  if( rq->struct_size != sizeof( vvr_ssim_request ) ) return outRefuse( c, "struct_size is not sizeof( vvr_ssim_request )", "vvr_ssim_submit" );
  vvr_compare_request q;
  memcpy( &q, rq, sizeof( q ) );
  return compareSubmit( c, &q, "vvr_ssim_submit", true );
}
// (a vvr_msssim_request is a vvr_compare_request up to `result`, with `scales` in the first pad byte and no map)
static_assert( sizeof( vvr_msssim_request ) == 96 && sizeof( vvr_frame_msssim ) == 616 && offsetof( vvr_msssim_request, ref ) == offsetof( vvr_compare_request, ref ) &&
               offsetof( vvr_msssim_request, result ) == offsetof( vvr_compare_request, result ) && offsetof( vvr_msssim_request, result ) + sizeof( void* ) == sizeof( vvr_msssim_request ) &&
               VVR_MSSSIM_MAX_SCALES == MSSSIM_MAX_SCALES, "vvr_msssim_request mirrors vvr_compare_request up to result" );
VVR_API int vvr_msssim_submit( vvr_context* c, const vvr_msssim_request* rq )
{
  if( !c || !rq ) return VVR_ERR_PARAMETER;
  if( rq->struct_size != sizeof( vvr_msssim_request ) ) return outRefuse( c, "struct_size is not sizeof( vvr_msssim_request )", "vvr_msssim_submit" );
  if( rq->scales < 1 || rq->scales > VVR_MSSSIM_MAX_SCALES ) return outRefuse( c, "scales must be 1 .. 5", "vvr_msssim_submit" );
  vvr_compare_request q;
  memset( &q, 0, sizeof( q ) );
  memcpy( &q, rq, sizeof( *rq ) );
  q.map = nullptr;
  return compareSubmit( c, &q, "vvr_msssim_submit", false, rq->scales );
}
// (a vvr_xpsnr_request is a vvr_compare_request up to ref_stride_bytes, with temporal and filter in the pad bytes and block in pad2)
static_assert( sizeof( vvr_xpsnr_request ) == 136 && sizeof( vvr_frame_xpsnr ) == 128 && sizeof( vvr_xpsnr_block ) == sizeof( unsigned long long ) * XPSNR_REC_WORDS &&
               offsetof( vvr_xpsnr_request, ref ) == offsetof( vvr_compare_request, ref ) && offsetof( vvr_xpsnr_request, prev ) == offsetof( vvr_compare_request, result ) &&
               offsetof( vvr_xpsnr_block, act_spatial ) == 24 && offsetof( vvr_xpsnr_block, count ) == 40, "vvr_xpsnr_request mirrors vvr_compare_request up to the reference's strides" );
VVR_API int vvr_xpsnr_submit( vvr_context* c, const vvr_xpsnr_request* rq )
{
  if( !c || !rq ) return VVR_ERR_PARAMETER;
  if( rq->struct_size != sizeof( vvr_xpsnr_request ) ) return outRefuse( c, "struct_size is not sizeof( vvr_xpsnr_request )", "vvr_xpsnr_submit" );
  if( rq->temporal > 2 ) return outRefuse( c, "temporal must be 0, 1 or 2", "vvr_xpsnr_submit" );
  if( rq->filter > 2 ) return outRefuse( c, "filter must be 0, 1 or 2", "vvr_xpsnr_submit" );
  if( rq->block & 3 ) return outRefuse( c, "block must be 0 or a multiple of 4", "vvr_xpsnr_submit" );
  vvr_compare_request q;
  memset( &q, 0, sizeof( q ) );
  memcpy( &q, rq, offsetof( vvr_compare_request, result ) );
  q.result = (vvr_frame_compare*) rq->result; q.map = nullptr;
  const XpsnrAsk ask = { rq->temporal, rq->filter, rq->block, { rq->prev[0], rq->prev[1] }, { rq->prev_stride_bytes[0], rq->prev_stride_bytes[1] }, rq->blocks };
  return compareSubmit( c, &q, "vvr_xpsnr_submit", false, 0, &ask );
}
#undef OQCHK

VVR_API int vvr_output_test( vvr_context* c, int ticket )
{
  if( !c ) return VVR_ERR_PARAMETER;
  hipSetDevice( c->device );
  std::unique_lock<std::mutex> lk( c->mu );
  OutEntry* e = outFind( c, ticket );
  if( !e ) { c->setError( "vvr_output_test: unknown or retired ticket" ); return VVR_ERR_PARAMETER; }
  if( e->rc != VVR_OK ) return e->rc;
  if( e->queued && hipEventQuery( e->done ) != hipSuccess ) return VVR_NOT_READY;
  return outJobStatus( c, e->job, lk, false );
}

VVR_API int vvr_output_wait( vvr_context* c, int ticket )
{
  if( !c ) return VVR_ERR_PARAMETER;
  hipSetDevice( c->device );
  std::unique_lock<std::mutex> lk( c->mu );
  OutEntry* e = outFind( c, ticket );
  if( !e || e->state != OQ_FLIGHT ) { c->setError( "vvr_output_wait: unknown or retired ticket" ); return VVR_ERR_PARAMETER; }
  e->state = OQ_WAITING;       // (the entry is this thread's now)
  int rc = e->rc;
  lk.unlock();
  if( e->queued && hipEventSynchronize( e->done ) != hipSuccess ) rc = VVR_ERR_DEVICE;
  lk.lock();
  if( rc == VVR_ERR_DEVICE && e->rc == VVR_OK ) c->setError( "vvr_output_wait: hipEventSynchronize failed" );
  if( rc == VVR_OK ) rc = outJobStatus( c, e->job, lk, true );
  outTimeEnd( c, e->timed, e->timing, e->msScales ? e->msScales : 1 );        // (K_OUTPUT_FRAME or K_OUTPUT_RGB; K_HASH_ROWS; K_OUTPUT_MSSSIM, a launch per scale ...
  outTimeEnd( c, e->timed0, e->timing0, e->rescales );      // (K_COMPARE_RESCALE; K_OUTPUT_RESAMPLE)
  outTimeEnd( c, e->timed2, e->timing2 );      // ... and K_HASH_COMBINE; K_OUTPUT_STATS and K_OUTPUT_STATS_SUM; K_OUTPUT_COMPARE and K_OUTPUT_COMPARE_SUM; K_OUTPUT_SSIM and K_OUTPUT_SSIM_SUM; K_OUTPUT_MSSSIM_SUM)
  // the slot's reader is gone (the event is complete: a picture that overwrote the slot meanwhile, or a vvr_sync, has dropped it already)
  if( e->slot >= 0 ) { auto& v = c->slotExt[e->slot]; v.erase( std::remove( v.begin(), v.end(), e->read ), v.end() ); }
  if( e->refSlot >= 0 ) { auto& v = c->slotExt[e->refSlot]; v.erase( std::remove( v.begin(), v.end(), e->read ), v.end() ); }      // (a comparison reads two slots)
  lk.unlock();
  if( rc == VVR_OK && e->queued && !e->direct )
    for( int k = 0; k < e->nc; k++ )
      for( int i = 0; i < e->count; i++ )
        for( int r = 0; r < e->rows[k]; r++ )
          memcpy( (uint8_t*) e->dst[k] + (size_t) i * e->bstride[k] + (size_t) r * e->dstStride[k], e->host + e->off[k] + (size_t) i * e->step[k] + (size_t) r * e->rowBytes[k], e->rowBytes[k] );
  if( rc == VVR_OK && e->queued && e->hash )
  {
    // the digests in vvr_picture_hash's byte order (MD5: the planes' bytes are hashed here, on the waiting thread), then the comparison with the SEI's
    const int method = e->hash - 1, len = method == VVR_HASH_MD5 ? 16 : method == VVR_HASH_CRC ? 2 : 4;
    uint8_t dg[48];
    for( int k = 0; k < e->hashNc; k++ )
    {
      uint8_t* out = dg + k * len;
      if( method == VVR_HASH_MD5 ) { Md5 m; m.update( (const uint8_t*) e->host + e->off[k], e->planeBytes[k] ); m.finish( out ); continue; }
      const uint32_t v = ( (const uint32_t*) e->host )[k];
      for( int i = 0; i < len; i++ ) out[i] = (uint8_t) ( v >> ( 8 * ( len - 1 - i ) ) );
    }
    if( e->digest ) memcpy( e->digest, dg, (size_t) e->hashNc * len );
    if( e->verify ) { uint32_t m = 0; for( int k = 0; k < e->hashNc; k++ ) if( memcmp( dg + k * len, e->expected + k * len, len ) ) m |= 1u << k; *e->mismatch = m; }
  }
  if( rc == VVR_OK && e->queued && e->stats )
  {
    // the caller's vvr_frame_stats: the header fields and the words (the minimum was accumulated as the maximum of M - v)
    const uint32_t* w = (const uint32_t*) e->host;
    vvr_frame_stats& st = *e->statsOut;
    memset( &st, 0, sizeof( st ) );
    st.struct_size = sizeof( st ); st.mode = (uint32_t) ( e->stats - 1 ); st.bit_depth = (uint32_t) c->cfg.bit_depth;
    st.width = (uint32_t) e->statsW; st.height = (uint32_t) e->statsH; st.samples = (uint64_t) e->statsW * e->statsH;
    memcpy( st.hist_y, w, sizeof( st.hist_y ) );
    if( st.mode == VVR_STATS_RGB )
    {
      memcpy( st.hist_maxrgb, w + 1024, sizeof( st.hist_maxrgb ) );
      for( int k = 0; k < 3; k++ ) { st.max_c[k] = w[2048 + k]; st.min_c[k] = ( ( 1u << c->cfg.bit_depth ) - 1 ) - w[2051 + k]; }
    }
  }
  if( rc == VVR_OK && e->queued && e->cmp && e->xps )
  {
    // the caller's vvr_frame_xpsnr: the header fields, the geometry and the sums over the records; the records as they lie
    const vvr_xpsnr_block* b = (const vvr_xpsnr_block*) e->host;
    const size_t n = (size_t) e->xpsBx * e->xpsBy;
    vvr_frame_xpsnr r;
    memset( &r, 0, sizeof( r ) );
    r.struct_size = sizeof( r ); r.bit_depth = (uint32_t) c->cfg.bit_depth; r.num_components = (uint32_t) e->cmp; r.temporal = (uint32_t) e->xpsTemporal;
    r.filter = (uint32_t) e->xpsFilter; r.block = (uint32_t) e->xpsBlock; r.blocks_x = (uint32_t) e->xpsBx; r.blocks_y = (uint32_t) e->xpsBy;
    for( int k = 0; k < e->cmp; k++ ) { r.width[k] = (uint32_t) ( e->cmpW >> ( k ? 1 : 0 ) ); r.height[k] = (uint32_t) ( e->cmpH >> ( k ? 1 : 0 ) ); r.samples[k] = (uint64_t) r.width[k] * r.height[k]; }
    for( size_t i = 0; i < n; i++ )
    {
      for( int k = 0; k < 3; k++ ) r.sse[k] += b[i].sse[k];
      r.act_spatial += b[i].act_spatial; r.act_temporal += b[i].act_temporal; r.count += b[i].count;
    }
    memcpy( (void*) e->cmpOut, &r, sizeof( r ) );
    if( e->xpsBlocks ) memcpy( e->xpsBlocks, b, sizeof( vvr_xpsnr_block ) * n );
  }
  else if( rc == VVR_OK && e->queued && e->cmp && e->msScales )
  {
    // the caller's vvr_frame_msssim: the header fields, per level and component the plane, the grid of windows and the two folded sums
    const uint32_t* w = (const uint32_t*) e->host;
    vvr_frame_msssim r;
    memset( &r, 0, sizeof( r ) );
    r.struct_size = sizeof( r ); r.bit_depth = (uint32_t) c->cfg.bit_depth; r.num_components = (uint32_t) e->cmp; r.scales = (uint32_t) e->msScales;
    for( int l = 0; l < e->msScales; l++ )
      for( int k = 0; k < e->cmp; k++ )
      {
        const uint32_t* o = w + ( l * e->cmp + k ) * MSSSIM_OUT_WORDS;
        r.width[l][k] = (uint32_t) ( ( e->cmpW >> ( k ? 1 : 0 ) ) >> l ); r.height[l][k] = (uint32_t) ( ( e->cmpH >> ( k ? 1 : 0 ) ) >> l );
        r.windows_x[l][k] = r.width[l][k] >= 8 ? ( r.width[l][k] - 8 ) / 4 + 1 : 0; r.windows_y[l][k] = r.height[l][k] >= 8 ? ( r.height[l][k] - 8 ) / 4 + 1 : 0;
        r.windows[l][k] = (uint64_t) r.windows_x[l][k] * r.windows_y[l][k];
        r.sum_cs[l][k] = (int64_t) ( o[0] | (uint64_t) o[1] << 32 ); r.sum_v[l][k] = (int64_t) ( o[2] | (uint64_t) o[3] << 32 );
      }
    memcpy( (void*) e->cmpOut, &r, sizeof( r ) );
  }
  else if( rc == VVR_OK && e->queued && e->cmp && e->cmpSsim )
  {
    // the caller's vvr_frame_ssim: the header fields, the grid of windows, the folded words - the key taken apart into the smallest v and the
    // origin of the first window that has it; the map
    const uint32_t* w = (const uint32_t*) e->host;
    vvr_frame_ssim r;
    memset( &r, 0, sizeof( r ) );
    r.struct_size = sizeof( r ); r.bit_depth = (uint32_t) c->cfg.bit_depth; r.num_components = (uint32_t) e->cmp;
    for( int k = 0; k < 3; k++ )
    {
      r.min[k] = 0x7fffffff; r.min_x[k] = r.min_y[k] = 0xffffffffu;
      if( k >= e->cmp ) continue;
      const uint32_t* o = w + k * SSIM_OUT_WORDS;
      r.width[k] = (uint32_t) ( e->cmpW >> ( k ? 1 : 0 ) ); r.height[k] = (uint32_t) ( e->cmpH >> ( k ? 1 : 0 ) );
      r.windows_x[k] = r.width[k] >= 8 ? ( r.width[k] - 8 ) / 4 + 1 : 0; r.windows_y[k] = r.height[k] >= 8 ? ( r.height[k] - 8 ) / 4 + 1 : 0;
      r.windows[k] = (uint64_t) r.windows_x[k] * r.windows_y[k];
      if( !r.windows[k] ) continue;
      r.sum[k] = (int64_t) ( o[0] | (uint64_t) o[1] << 32 ); r.min[k] = (int32_t) ( o[3] ^ 0x80000000u );
      r.min_x[k] = 4 * ( o[2] % r.windows_x[k] ); r.min_y[k] = 4 * ( o[2] / r.windows_x[k] );
    }
    memcpy( (void*) e->cmpOut, &r, sizeof( r ) );
    if( e->cmpMap ) memcpy( e->cmpMap, w + CMP_HEAD_WORDS, sizeof( uint32_t ) * e->cmpBlocks );
  }
  else if( rc == VVR_OK && e->queued && e->cmp )
  {
    // the caller's vvr_frame_compare: the header fields, the folded words, the first index as a position in the component's window; the map
    const uint32_t* w = (const uint32_t*) e->host;
    vvr_frame_compare& r = *e->cmpOut;
    memset( &r, 0, sizeof( r ) );
    r.struct_size = sizeof( r ); r.bit_depth = (uint32_t) c->cfg.bit_depth; r.num_components = (uint32_t) e->cmp;
    for( int k = 0; k < 3; k++ )
    {
      r.first_x[k] = r.first_y[k] = 0xffffffffu;
      if( k >= e->cmp ) continue;
      const uint32_t* o = w + k * CMP_OUT_WORDS;
      r.width[k] = (uint32_t) ( e->cmpW >> ( k ? 1 : 0 ) ); r.height[k] = (uint32_t) ( e->cmpH >> ( k ? 1 : 0 ) ); r.samples[k] = (uint64_t) r.width[k] * r.height[k];
      r.sse[k] = o[0] | (uint64_t) o[1] << 32; r.sad[k] = o[2] | (uint64_t) o[3] << 32; r.differing[k] = o[4] | (uint64_t) o[5] << 32; r.max_abs[k] = o[6];
      if( o[7] != 0xffffffffu ) { r.first_x[k] = o[7] % r.width[k]; r.first_y[k] = o[7] / r.width[k]; }
    }
    if( e->cmpMap ) memcpy( e->cmpMap, w + CMP_HEAD_WORDS, sizeof( uint32_t ) * e->cmpBlocks );
  }
  lk.lock();
  e->state = OQ_FREE; e->ticket = -1;
  return rc;
}

VVR_API int vvr_output_stream_wait( vvr_context* c, int ticket, void* stream )
{
  if( !c ) return VVR_ERR_PARAMETER;
  hipSetDevice( c->device );
  std::unique_lock<std::mutex> lk( c->mu );
  OutEntry* e = outFind( c, ticket );
  if( !e || e->state != OQ_FLIGHT ) { c->setError( "vvr_output_stream_wait: unknown or retired ticket" ); return VVR_ERR_PARAMETER; }
  if( e->rc != VVR_OK ) return e->rc;      // (the request's job had failed, or its copy could not be enqueued: nothing to wait for)
  if( e->queued ) HIPCHK( c, hipStreamWaitEvent( (hipStream_t) stream, e->done, 0 ) );
  return VVR_OK;
}

VVR_API void* vvr_device_alloc( vvr_context* c, size_t bytes )
{
  if( !c || !bytes ) return nullptr;
  hipSetDevice( c->device );
  void* p = nullptr;
  if( hipMalloc( &p, bytes ) != hipSuccess ) return nullptr;
  std::lock_guard<std::mutex> lk( c->mu );
  c->devRanges.push_back( DevRange{ (char*) p, bytes, true } );
  return p;
}

VVR_API int vvr_device_register( vvr_context* c, void* p, size_t bytes )
{
  if( !c ) return VVR_ERR_PARAMETER;
  std::lock_guard<std::mutex> lk( c->mu );
  if( !p || !bytes ) { c->setError( "vvr_device_register: no pointer or no bytes" ); return VVR_ERR_PARAMETER; }
  for( const DevRange& r : c->devRanges )
    if( (char*) p < r.p + r.n && (char*) p + bytes > r.p ) { c->setError( "vvr_device_register: the range overlaps one that is registered or allocated already" ); return VVR_ERR_PARAMETER; }
  c->devRanges.push_back( DevRange{ (char*) p, bytes, false } );
  return VVR_OK;
}

namespace {
// the range that starts at p, and whether a request whose ticket has not been retired writes into it.  mu held.
int devRangeAt( vvr_context* c, const void* p, bool& busy )
{
  busy = false;
  int at = -1;
  for( size_t i = 0; i < c->devRanges.size(); i++ ) if( c->devRanges[i].p == (const char*) p ) at = (int) i;
  if( at < 0 || !c->outRing ) return at;
  const DevRange& r = c->devRanges[at];
  for( int i = 0; i < VVR_OUT_RING; i++ )
  {
    const OutEntry& e = c->outRing[i];
    if( e.state == OQ_FREE || !e.devDst ) continue;
    for( int k = 0; k < e.nc; k++ ) if( (const char*) e.dst[k] >= r.p && (const char*) e.dst[k] + e.extent[k] <= r.p + r.n ) busy = true;
  }
  return at;
}
}   // namespace

VVR_API int vvr_device_unregister( vvr_context* c, void* p )
{
  if( !c ) return VVR_ERR_PARAMETER;
  std::lock_guard<std::mutex> lk( c->mu );
  bool busy;
  const int at = devRangeAt( c, p, busy );
  if( at < 0 || c->devRanges[at].owned ) { c->setError( at < 0 ? "vvr_device_unregister: unknown pointer" : "vvr_device_unregister: memory of vvr_device_alloc (vvr_device_free gives it back)" ); return VVR_ERR_PARAMETER; }
  if( busy ) { c->setError( "vvr_device_unregister: a request in flight writes into the range (vvr_output_wait retires it)" ); return VVR_ERR_BUSY; }
  c->devRanges.erase( c->devRanges.begin() + at );
  return VVR_OK;
}

VVR_API void vvr_device_free( vvr_context* c, void* p )
{
  if( !c ) return;
  hipSetDevice( c->device );
  std::unique_lock<std::mutex> lk( c->mu );
  bool busy;
  const int at = devRangeAt( c, p, busy );
  if( at < 0 || !c->devRanges[at].owned ) { c->setError( at < 0 ? "vvr_device_free: unknown pointer" : "vvr_device_free: registered memory of the caller's (vvr_device_unregister)" ); return; }
  c->devRanges.erase( c->devRanges.begin() + at );
  hipStream_t s = c->outQStream;
  lk.unlock();
  if( busy && s ) hipStreamSynchronize( s );      // (behind the request that writes it; its ticket stays)
  hipFree( p );
}

}   // extern "C"
