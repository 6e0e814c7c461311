// invaug.hip -- per-sample dihedral transform of the last two axes (the geometric part of the reference's
// transform/invertible_augmentations.py: kornia's RandomHorizontalFlip / RandomVerticalFlip / RandomRotation90 and their
// inverses, which the reference runs as a 2-D warp per sample).  A flip / 90-degree-rotation chain composes to one of the eight
// elements of D4, a pure permutation: one pass, a bit copy of 1-, 2- or 4-byte elements, one code per sample.
//
// Code c (include/tem_hip.h): bit 0 transposes, bit 1 reverses the source row, bit 2 reverses the source column;
// dst[n,p,i,j] = src[n,p,r,s] with (r, s) = bit 0 ? (j, i) : (i, j), then r = H-1-r (bit 1), s = W-1-s (bit 2).
//
// One launch serves a batch of mixed codes: a workgroup works on ONE sample (blockIdx.x / blocks-per-sample), reads that
// sample's code once (a scalar load) and branches on it, so every branch is wave-uniform.
//   * codes 0, 2, 4, 6 stream: 16-byte loads and stores along rows; a column reversal reads the mirrored 16-byte chunk and
//     reverses its elements in registers.  Rows that are no multiple of 16 bytes, or a base off a 16-byte boundary, go
//     element by element (the scalar stream).
//   * codes 1, 3, 5, 7 go tile by tile through LDS: a 32 x 32 tile is read along source rows and written along destination
//     rows, so both global sides are row-contiguous.  The tile is [32][33] dwords: ds_write / ds_read_b32 bank on
//     (addr / 4) % 32, and the column read of an unpadded 32-dword pitch would be a 32-way conflict.  1- and 2-byte
//     elements take tiles of 128 / 64 elements a side, packed, so that a lane moves a dword on both global sides
//     (dh_tile_packed); where their rows or bases are not dword-aligned they are widened to one LDS dword each instead.
// Indices into the tensors are 64-bit; the stream paths divide in 32 bits when a sample's unit count allows it.
#include "tem_common.h"

#define DH_PATH_VEC 0
#define DH_PATH_SCALAR 1
#define DH_PATH_TILE 2
#define DH_PATH_TILE_PACKED 3
#define DH_TILE 32
#define DH_ROWS 8   // tile rows per pass of the 256 threads

template <int EB> struct dh_elem;
template <> struct dh_elem<1> { typedef uint8_t type; };
template <> struct dh_elem<2> { typedef uint16_t type; };
template <> struct dh_elem<4> { typedef uint32_t type; };

// the 16 / EB elements of a 16-byte chunk in reverse order
template <int EB> __device__ __forceinline__ uint4 dh_reverse16(uint4 v) {
    uint4 r = make_uint4(v.w, v.z, v.y, v.x);
    if constexpr (EB == 2) {
        r.x = (r.x >> 16) | (r.x << 16); r.y = (r.y >> 16) | (r.y << 16);
        r.z = (r.z >> 16) | (r.z << 16); r.w = (r.w >> 16) | (r.w << 16);
    }
    if constexpr (EB == 1) {
        r.x = __builtin_bswap32(r.x); r.y = __builtin_bswap32(r.y);
        r.z = __builtin_bswap32(r.z); r.w = __builtin_bswap32(r.w);
    }
    return r;
}

// One sample, non-transposing: `rows` = planes * H rows of `wu` units each (16-byte chunks, or elements); unit q of the
// destination comes from row `mirrored row within its plane` (fr) and unit wu-1-v (fc).  I: the index type of the divisions.
template <typename U, int EB, bool VEC, typename I>
__device__ __forceinline__ void dh_stream(const U* __restrict__ s, U* __restrict__ d, I rows, I H, I wu, bool fr, bool fc,
                                          I first, I step) {
    const I n = rows * wu;
    for (I q = first; q < n; q += step) {
        const I row = q / wu, v = q - row * wu;
        I srow = row;
        if (fr) {
            const I p = row / H;
            srow = p * H + (H - 1 - (row - p * H));
        }
        U x = s[srow * wu + (fc ? wu - 1 - v : v)];
        if constexpr (VEC) {
            if (fc) x = dh_reverse16<EB>(x);
        }
        d[q] = x;
    }
}

// One sample, transposing: the destination plane is [W][H]; tile (i0, j0) of it holds source rows r(j), columns s(i).
// 32 x 32 elements, one per LDS dword (4-byte elements, and narrow ones whose rows or bases are not dword-aligned).
template <int EB>
__device__ __forceinline__ void dh_tile(const typename dh_elem<EB>::type* __restrict__ s, typename dh_elem<EB>::type* __restrict__ d,
                                        int planes, int H, int W, bool fr, bool fc, int b, int bps, uint32_t (*tile)[DH_TILE + 1]) {
    typedef typename dh_elem<EB>::type T;
    const int64_t tJ = ((int64_t)H + DH_TILE - 1) / DH_TILE, tI = ((int64_t)W + DH_TILE - 1) / DH_TILE;
    const int64_t per_plane = tI * tJ, nt = per_plane * planes;
    const int tx = threadIdx.x & (DH_TILE - 1), ty = threadIdx.x / DH_TILE;
    for (int64_t t = b; t < nt; t += bps) {   // trip count is block-uniform: the barriers below are reached by all threads
        const int64_t p = t / per_plane, rem = t - p * per_plane;
        const int64_t i0 = (rem / tJ) * DH_TILE, j0 = (rem % tJ) * DH_TILE;
        const T* sp = s + p * H * W;
        T* dp = d + p * H * W;
        {
            const int64_t i = i0 + tx, col = fc ? W - 1 - i : i;
#pragma unroll
            for (int a = ty; a < DH_TILE; a += DH_ROWS) {
                const int64_t j = j0 + a;
                if (i < W && j < H) tile[a][tx] = sp[(fr ? H - 1 - j : j) * W + col];
            }
        }
        __syncthreads();
        {
            const int64_t j = j0 + tx;
#pragma unroll
            for (int a = ty; a < DH_TILE; a += DH_ROWS) {
                const int64_t i = i0 + a;
                if (i < W && j < H) dp[i * H + j] = (T)tile[tx][a];
            }
        }
        __syncthreads();
    }
}

// The same for 1- and 2-byte elements with H, W multiples of EPD = 4 / EB and dword-aligned bases: tiles of TE = 32 * EPD
// elements a side, so a lane moves a whole dword on both global sides (64 lanes x 2 bytes are half a cache line per wave
// instruction; profiles/invaug_bench.txt has both variants).  A loaded dword holds EPD consecutive source columns = EPD
// destination rows (in reverse order under a column reversal: the dword's elements are reversed first); they are written
// element by element into the DESTINATION-major tile [TE][TE + EPD], and the store phase reads whole dwords along a
// destination row.  Banks: the dword reads are conflict-free (consecutive lanes, consecutive dwords); the element writes of
// a 32-lane group land (pitch 33 dwords, EPD rows per lane) EPD lanes to a bank, which a store absorbs at EPD = 2.
template <int EB>
__device__ __forceinline__ void dh_tile_packed(const typename dh_elem<EB>::type* __restrict__ s, typename dh_elem<EB>::type* __restrict__ d,
                                               int planes, int H, int W, bool fr, bool fc, int b, int bps,
                                               typename dh_elem<EB>::type* __restrict__ tile) {
    typedef typename dh_elem<EB>::type T;
    constexpr int EPD = 4 / EB, TE = DH_TILE * EPD, P = TE + EPD;
    const int64_t tJ = ((int64_t)H + TE - 1) / TE, tI = ((int64_t)W + TE - 1) / TE;
    const int64_t per_plane = tI * tJ, nt = per_plane * planes;
    const int tx = threadIdx.x & (DH_TILE - 1), ty = threadIdx.x / DH_TILE;
    for (int64_t t = b; t < nt; t += bps) {
        const int64_t p = t / per_plane, rem = t - p * per_plane;
        const int64_t i0 = (rem / tJ) * TE, j0 = (rem % tJ) * TE;
        const T* sp = s + p * H * W;
        T* dp = d + p * H * W;
        {
            const int64_t i = i0 + tx * EPD;               // the first of this lane's EPD destination rows
            const int64_t col = fc ? W - EPD - i : i;      // the dword's first source column (W % EPD == 0)
            for (int a = ty; a < TE; a += DH_ROWS) {
                const int64_t j = j0 + a;
                if (i < W && j < H) {
                    uint32_t v = *reinterpret_cast<const uint32_t*>(sp + (fr ? H - 1 - j : j) * W + col);
                    if (fc) v = EB == 2 ? (v >> 16) | (v << 16) : __builtin_bswap32(v);
#pragma unroll
                    for (int e = 0; e < EPD; ++e) tile[(tx * EPD + e) * P + a] = (T)(v >> (8 * EB * e));
                }
            }
        }
        __syncthreads();
        {
            const int64_t j = j0 + tx * EPD;
            for (int a = ty; a < TE; a += DH_ROWS) {
                const int64_t i = i0 + a;
                if (i < W && j < H) *reinterpret_cast<uint32_t*>(dp + i * H + j) = *reinterpret_cast<const uint32_t*>(tile + a * P + tx * EPD);
            }
        }
        __syncthreads();
    }
}

template <int EB> struct dh_lds {   // dwords: the 32 x 33 tile, or the packed tile of narrow elements when that is larger
    static constexpr int EPD = 4 / EB, PACKED = EB < 4 ? (DH_TILE * EPD) * (DH_TILE * EPD + EPD) / EPD : 0;
    static constexpr int DWORDS = PACKED > DH_TILE * (DH_TILE + 1) ? PACKED : DH_TILE * (DH_TILE + 1);
};

template <int EB>
__global__ __launch_bounds__(256) void k_dihedral2d(const void* __restrict__ src, void* __restrict__ dst, const int* __restrict__ codes,
                                                    int planes, int H, int W, int bps, int vec, int packed) {
    typedef typename dh_elem<EB>::type T;
    __shared__ uint32_t lds[dh_lds<EB>::DWORDS];
    const int n = blockIdx.x / bps, b = blockIdx.x - n * bps;
    const int code = codes[n] & 7;   // block-uniform: one scalar load
    const bool fr = code & 2, fc = code & 4;
    const int64_t S = (int64_t)planes * H * W;   // elements per sample
    const T* s = (const T*)src + (int64_t)n * S;
    T* d = (T*)dst + (int64_t)n * S;
    if (!(code & 1)) {
        const int64_t rows = (int64_t)planes * H;
        const int64_t wu = vec ? (int64_t)W * EB / 16 : W;
        const int64_t first = (int64_t)b * 256 + threadIdx.x, step = (int64_t)bps * 256;
        const bool small = rows * wu < ((int64_t)1 << 31);   // q + step stays below 2^32: step <= 2048 * 256
        if (vec) {
            if (small) dh_stream<uint4, EB, true, uint32_t>((const uint4*)s, (uint4*)d, (uint32_t)rows, (uint32_t)H, (uint32_t)wu, fr, fc, (uint32_t)first, (uint32_t)step);
            else dh_stream<uint4, EB, true, int64_t>((const uint4*)s, (uint4*)d, rows, (int64_t)H, wu, fr, fc, first, step);
        } else {
            if (small) dh_stream<T, EB, false, uint32_t>(s, d, (uint32_t)rows, (uint32_t)H, (uint32_t)wu, fr, fc, (uint32_t)first, (uint32_t)step);
            else dh_stream<T, EB, false, int64_t>(s, d, rows, (int64_t)H, wu, fr, fc, first, step);
        }
        return;
    }
    if constexpr (EB < 4) {
        if (packed) {
            dh_tile_packed<EB>(s, d, planes, H, W, fr, fc, b, bps, (T*)lds);
            return;
        }
    }
    dh_tile<EB>(s, d, planes, H, W, fr, fc, b, bps, (uint32_t(*)[DH_TILE + 1]) lds);
}

// ---- one plan for the query and the launch ----------------------------------------------------------------------------
static int dh_check(const char* who, const void* src, const void* dst, int N, int planes, int H, int W, int eb) {
    TEM_REQUIRE(src && dst, "%s: null pointer", who);
    TEM_REQUIRE(N > 0 && planes > 0 && H > 0 && W > 0, "%s: bad sizes (N=%d planes=%d H=%d W=%d)", who, N, planes, H, W);
    TEM_REQUIRE(eb == 1 || eb == 2 || eb == 4, "%s: elem_bytes must be 1, 2 or 4, got %d", who, eb);
    TEM_REQUIRE((double)N * planes * H * W * eb < 9.0e18, "%s: the tensor is too large", who);
    const int64_t bytes = (int64_t)N * planes * H * W * eb;
    TEM_REQUIRE((const char*)dst + bytes <= (const char*)src || (const char*)src + bytes <= (const char*)dst,
                "%s: in-place or overlapping src / dst (a permutation cannot run in place)", who);
    return TEM_OK;
}

static bool dh_vec(const void* src, const void* dst, int W, int eb) {
    return ((int64_t)W * eb) % 16 == 0 && (uintptr_t)src % 16 == 0 && (uintptr_t)dst % 16 == 0;
}

// narrow elements whose rows (of source and destination: W and H) and bases are dword-aligned take the packed tile
static bool dh_packed(const void* src, const void* dst, int H, int W, int eb) {
    return eb < 4 && W % (4 / eb) == 0 && H % (4 / eb) == 0 && (uintptr_t)src % 4 == 0 && (uintptr_t)dst % 4 == 0;
}

extern "C" int tem_dihedral2d_path(const void* src, const void* dst, int code, int N, int planes, int H, int W, int elem_bytes) {
    if (dh_check("tem_dihedral2d_path", src, dst, N, planes, H, W, elem_bytes) != TEM_OK) return -1;
    if (code < 0 || code > 7) {
        tem_set_error("tem_dihedral2d_path: code %d is outside 0..7", code);
        return -1;
    }
    if (code & 1) return dh_packed(src, dst, H, W, elem_bytes) ? DH_PATH_TILE_PACKED : DH_PATH_TILE;
    return dh_vec(src, dst, W, elem_bytes) ? DH_PATH_VEC : DH_PATH_SCALAR;
}

extern "C" int tem_dihedral2d(const void* src, void* dst, const int* codes_dev, int N, int planes, int H, int W, int elem_bytes,
                              tem_stream_t stream) {
    TEM_TRY(dh_check("tem_dihedral2d", src, dst, N, planes, H, W, elem_bytes));
    TEM_REQUIRE(codes_dev, "tem_dihedral2d: null pointer");
    // blocks per sample: one per 4 KiB (a pass of 256 x 16 bytes, or a 32 x 32 tile of dwords), about 2048 in the whole grid
    const int64_t sample_bytes = (int64_t)planes * H * W * elem_bytes;
    const int bps = tem_grid_1d(tem_cdiv(sample_bytes, 4096), 1, N >= 2048 ? 1 : 2048 / N);
    const int vec = dh_vec(src, dst, W, elem_bytes) ? 1 : 0, packed = dh_packed(src, dst, H, W, elem_bytes) ? 1 : 0;
    const dim3 grid((unsigned)((int64_t)N * bps));   // N * bps <= max(N, 2048) < 2^31
    const hipStream_t st = (hipStream_t)stream;
    if (elem_bytes == 4) hipLaunchKernelGGL((k_dihedral2d<4>), grid, dim3(256), 0, st, src, dst, codes_dev, planes, H, W, bps, vec, packed);
    else if (elem_bytes == 2) hipLaunchKernelGGL((k_dihedral2d<2>), grid, dim3(256), 0, st, src, dst, codes_dev, planes, H, W, bps, vec, packed);
    else hipLaunchKernelGGL((k_dihedral2d<1>), grid, dim3(256), 0, st, src, dst, codes_dev, planes, H, W, bps, vec, packed);
    TEM_CHECK_LAUNCH("tem_dihedral2d");
    return TEM_OK;
}
