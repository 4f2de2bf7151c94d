// "4 pixels per lane and step": the memory accesses and the wavefront tail that the counting kernels share (stq_ops.hip, tc_ops.hip,
// flow_occ_ops.hip, flow_err_ops.hip, sseg_confusion_kernel of ipq_ops.hip). Chunk ch holds pixels 4 ch .. 4 ch + n - 1 (linear index,
// n < 4 only in the last one). Everything that decides whether a kernel reads or writes outside a buffer is here, once.
// Part A is integer and address work only and also compiles as plain C++: tests/test_px4_host.py runs it under the host sanitizers.
// Part C is how a workgroup's counters and sums reach the caller's tables (flow_occ, flow_err, flow_photo, flow_census): once.
#pragma once
#include <stdint.h>
#ifdef __HIPCC__
#include "common.h"
#define PX4_FN __device__ __forceinline__
#define px4_alignbyte(hi, lo, o) __builtin_amdgcn_alignbyte(hi, lo, o)
#else
#define PX4_FN static inline
#define px4_alignbyte(hi, lo, o) ((uint32_t)(((((uint64_t)(hi)) << 32) | (lo)) >> (8 * (o))))
#endif

// ---------------------------------------------------------------------------------------------- Part A: loads, stores, search
constexpr int PX4 = 4;

typedef uint32_t __attribute__((may_alias)) px4_u32;
struct __attribute__((aligned(8), may_alias)) px4_f2 { float x, y; };
struct __attribute__((aligned(16), may_alias)) px4_f4 { float x, y, z, w; };

// How a flow of `ld` floats per pixel with its two channels at `coff` is loaded (host): 2 = dense [h,w,2] on a 16-byte boundary, two
// 16-byte loads per chunk; 1 = every pixel's pair on an 8-byte boundary, one 8-byte load each; 0 = two 4-byte loads each.
static inline int px4_flow_mode(const float* f, int ld, int coff) {
    return (ld == 2 && coff == 0 && ((uintptr_t)f & 15) == 0) ? 2 : ((ld & 1) == 0 && ((uintptr_t)(f + coff) & 7) == 0) ? 1 : 0;
}

// pixels p0 .. p0 + n - 1 of a flow, by px4_flow_mode's `fmode`; u and v of the pixels past n are 0
PX4_FN void px4_load_flow(const float* __restrict__ f, int ld, int coff, int fmode, long p0, int n, float (&u)[PX4], float (&v)[PX4]) {
    if (fmode == 2 && n == PX4) {
        const px4_f4 f0 = *reinterpret_cast<const px4_f4*>(f + 2 * p0), f1 = *reinterpret_cast<const px4_f4*>(f + 2 * p0 + 4);
        u[0] = f0.x; v[0] = f0.y; u[1] = f0.z; v[1] = f0.w; u[2] = f1.x; v[2] = f1.y; u[3] = f1.z; v[3] = f1.w;
        return;
    }
#pragma unroll
    for (int i = 0; i < PX4; ++i) {
        u[i] = v[i] = 0.f;
        if (i < n) {
            const float* q = f + (p0 + i) * ld + coff;
            if (fmode >= 1) { const px4_f2 g = *reinterpret_cast<const px4_f2*>(q); u[i] = g.x; v[i] = g.y; }
            else { u[i] = q[0]; v[i] = q[1]; }
        }
    }
}

// The three bytes (as one 24-bit value, channel 0 lowest) of the pixels of chunk ch of a [npix][3] byte map (nbytes = 3 npix) whose base
// need not be dword-aligned: the 12 bytes sit in 3 aligned dwords (4 when the base is off a dword boundary), loaded as dwords and shifted
// into place. A chunk whose dwords would reach in front of the base or past byte nbytes (the first one of an unaligned map, the last one
// or two of any map) is read byte by byte; pixels past n are 0 there.
PX4_FN void px4_load_px3(const uint8_t* __restrict__ p, long nbytes, long ch, int n, uint32_t (&px)[PX4]) {
    const unsigned o = (unsigned)((uintptr_t)p & 3);
    const long b0 = 12 * ch;                          // first byte of the chunk's dwords, counted from the aligned address p - o
    if (b0 >= (long)o && b0 + (o ? 16 : 12) <= (long)o + nbytes) {
        const px4_u32* w = reinterpret_cast<const px4_u32*>(p - o) + 3 * ch;
        const uint32_t w0 = w[0], w1 = w[1], w2 = w[2], w3 = o ? w[3] : 0u;
        const uint32_t d0 = px4_alignbyte(w1, w0, o), d1 = px4_alignbyte(w2, w1, o), d2 = px4_alignbyte(w3, w2, o);
        px[0] = d0 & 0xffffffu;
        px[1] = (d0 >> 24) | ((d1 & 0xffffu) << 8);
        px[2] = (d1 >> 16) | ((d2 & 0xffu) << 16);
        px[3] = d2 >> 8;
    } else {
#pragma unroll
        for (int i = 0; i < PX4; ++i) {
            px[i] = 0;
            if (i < n) {
                const uint8_t* a = p + b0 + 3 * i;
                px[i] = a[0] | (a[1] << 8) | (a[2] << 16);
            }
        }
    }
}

// bytes p0 .. p0 + n - 1 of a [npix] byte map whose base need not be dword-aligned (p0 is a multiple of 4), byte i in bits 8 i: one aligned
// dword, or two aligned dwords shifted into place when the base is off a dword boundary. A chunk whose dwords would reach in front of
// the base or past byte npix is read byte by byte.
PX4_FN uint32_t px4_load_bytes(const uint8_t* __restrict__ p, long npix, long p0, int n) {
    const unsigned o = (unsigned)((uintptr_t)p & 3);
    if (n == PX4) {
        if (!o) return *reinterpret_cast<const px4_u32*>(p + p0);
        if (p0 >= 4 && p0 - (long)o + 8 <= npix) {
            const px4_u32* w = reinterpret_cast<const px4_u32*>(p + p0 - o);
            return px4_alignbyte(w[1], w[0], o);
        }
    }
    uint32_t r = 0;
#pragma unroll
    for (int i = 0; i < PX4; ++i)
        if (i < n) r |= (uint32_t)p[p0 + i] << (8 * i);
    return r;
}

// bytes p0 .. p0 + n - 1 of a byte map for ANY p0 (the 4 pixels of a lane inside a tile row), byte i in bits 8 i: one dword where the
// address p + p0 is dword-aligned and the chunk is whole, byte by byte otherwise. Only the n bytes themselves are read either way.
PX4_FN uint32_t px4_load_bytes_at(const uint8_t* __restrict__ p, long p0, int n) {
    if (n == PX4 && ((uintptr_t)(p + p0) & 3) == 0) return *reinterpret_cast<const px4_u32*>(p + p0);
    uint32_t r = 0;
#pragma unroll
    for (int i = 0; i < PX4; ++i)
        if (i < n) r |= (uint32_t)p[p0 + i] << (8 * i);
    return r;
}

// the other way: byte i of `codes` to dst[p0 + i], as one dword where dst is dword-aligned (dst4) and the chunk is whole
PX4_FN void px4_store_bytes(uint8_t* __restrict__ dst, bool dst4, long p0, int n, uint32_t codes) {
    if (dst4 && n == PX4) {
        *reinterpret_cast<px4_u32*>(dst + p0) = codes;
    } else {
        for (int i = 0; i < n; ++i) dst[p0 + i] = (uint8_t)(codes >> (8 * i));
    }
}

// the 24-bit values c (channel 0 lowest) to pixels p0 .. p0 + n - 1 of a [npix][3] byte map, as three dwords under the same condition
PX4_FN void px4_store_px3(uint8_t* __restrict__ dst, bool dst4, long p0, int n, const uint32_t (&c)[PX4]) {
    uint8_t* q = dst + 3 * p0;
    if (dst4 && n == PX4) {
        px4_u32* w = reinterpret_cast<px4_u32*>(q);
        w[0] = c[0] | (c[1] << 24);
        w[1] = (c[1] >> 8) | (c[2] << 16);
        w[2] = (c[2] >> 16) | (c[3] << 8);
    } else {
#pragma unroll
        for (int i = 0; i < PX4; ++i)
            if (i < n) { q[3 * i] = (uint8_t)c[i]; q[3 * i + 1] = (uint8_t)(c[i] >> 8); q[3 * i + 2] = (uint8_t)(c[i] >> 16); }
    }
}

// the place of v among n sorted, unique keys; n = not listed
template <class K>
PX4_FN int px4_sorted_index(const K* __restrict__ keys, int n, uint32_t v) {
    int lo = 0, hi = n - 1;
    while (lo <= hi) {
        const int mid = (lo + hi) >> 1;
        const uint32_t m = keys[mid];
        if (m == v) return mid;
        if (m < v) lo = mid + 1; else hi = mid - 1;
    }
    return n;
}

// ---------------------------------------------------------------------------------------------- Part B: the wavefront
#ifdef __HIPCC__
// the sum over the 64 lanes, in every lane (uint32_t, int, double): x(l) + x(l ^ off) for off = 32 .. 1, a fixed tree for the doubles
template <class T>
__device__ __forceinline__ T wave_sum(T x) {
    for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off, 64);
    return x;
}

// The run each lane is left with after its chunk (has, its state packed into key, len pixels long): true where every lane that has one
// holds the same key - the inside of a region. Then sum is their total length and src the first such lane, for one add per wavefront;
// otherwise (and where no lane has a run) every lane adds its own. All lanes of the wavefront call this together.
__device__ __forceinline__ bool wave_same_run(bool has, uint64_t key, uint32_t len, int& src, uint32_t& sum) {
    const unsigned long long act = __ballot(has);
    src = __ffsll((long long)act) - 1;
    sum = 0;
    if (!act) return false;
    const unsigned long long first = __shfl((unsigned long long)key, src, 64);
    if (__ballot(has && key != first)) return false;
    sum = wave_sum(has ? len : 0u);
    return true;
}
#endif

// ---------------------------------------------------------------------------------------------- Part C: the workgroup's tables
// How a lane's counters and sums leave a workgroup of PX4_WG lanes: summed over the wavefront into one LDS row per wavefront, then
// the counts as one 64-bit atomic per non-zero cell and the sums, without any floating-point atomic, as the workgroup's own slot.
constexpr int PX4_WG = 256;
constexpr int PX4_MAX_GROUPS = 1024;                  // workgroups of a launch with slots = slots of its workspace (4 per CU, then grid-stride)

static inline long px4_groups(long npix) {
    const long nchunk = (npix + PX4 - 1) / PX4, g = (nchunk + PX4_WG - 1) / PX4_WG;
    return g > PX4_MAX_GROUPS ? PX4_MAX_GROUPS : g;
}

static inline int64_t px4_slot_bytes(long groups, int nsum) { return (int64_t)(groups * nsum * sizeof(double)); }

#ifdef __HIPCC__
template <int N, class T>
__device__ __forceinline__ void wg_rows(const T (&cell)[N], T (&red)[PX4_WG / 64][N]) {
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const T s = wave_sum(cell[k]);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = s;
    }
    __syncthreads();
}

// T: uint32_t or unsigned long long; a workgroup's total of a cell fits it (the callers bound their pixels)
template <int NCELL, class T>
__device__ __forceinline__ void wg_counts_to_table(const T (&cell)[NCELL], T (&red)[PX4_WG / 64][NCELL], unsigned long long* __restrict__ table) {
    wg_rows(cell, red);
    if (threadIdx.x < NCELL) {
        T c = 0;
        for (int w = 0; w < PX4_WG / 64; ++w) c += red[w][threadIdx.x];
        if (c) atomicAdd(&table[threadIdx.x], (unsigned long long)c);
    }
}

// lanes 64 .. 64 + NSUM - 1 write the slot, zeros too: the finishing launch reads every slot
template <int NSUM>
__device__ __forceinline__ void wg_sums_to_slot(const double (&sum)[NSUM], double (&red)[PX4_WG / 64][NSUM], double* __restrict__ slots) {
    wg_rows(sum, red);
    if (threadIdx.x >= 64 && threadIdx.x < 64 + NSUM) {
        const int k = threadIdx.x - 64;
        slots[(long)blockIdx.x * NSUM + k] = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
    }
}

// ONE workgroup: lane t owns cell t % NSUM and adds the slots t / NSUM, + PX4_WG / NSUM, ... in ascending order; a cell's lanes are then
// summed in a fixed tree (xor shuffles over NSUM .. 32, then the four wavefronts in order) and the totals are added to `sums`.
template <int NSUM>
__global__ __launch_bounds__(PX4_WG)
void slot_finish_kernel(const double* __restrict__ slots, int nslots, double* __restrict__ sums) {
    static_assert(PX4_WG == 256 && NSUM <= 32 && (NSUM & (NSUM - 1)) == 0, "four wavefronts; a cell's lanes are an xor class");
    __shared__ double part[PX4_WG / 64][NSUM];
    const int k = threadIdx.x % NSUM;
    double s = 0.0;
    for (int j = threadIdx.x / NSUM; j < nslots; j += PX4_WG / NSUM) s += slots[(long)j * NSUM + k];
    for (int off = NSUM; off <= 32; off <<= 1) s += __shfl_xor(s, off, 64);
    if ((threadIdx.x & 63) < NSUM) part[threadIdx.x >> 6][k] = s;
    __syncthreads();
    if (threadIdx.x < NSUM) sums[k] = sums[k] + ((part[0][k] + part[1][k]) + (part[2][k] + part[3][k]));
}
#endif
