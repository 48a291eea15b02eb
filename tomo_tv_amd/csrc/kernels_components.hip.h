// kernels_components.hip.h -- connected-component labelling of a thresholded volume and the per-component measurements
// (tomo_components_*; engine_components.inc).  Part of kernels.hip.h (include that, not this).
//
// The label array L is NOT in the volume's [pix][sx] layout but in the public order: one int32 per real voxel at the public linear
// index p = (s N + y) N + z (no padding slices), so that "the smallest index wins" is at once the union-find rule, the component's
// `first` and the numbering order, and tomo_components_get_labels is a plain copy.  Only k_cc_init and k_cc_keep touch a volume; both
// go through a 64 x 64 LDS tile like k_dart_state_out, so that the volume is accessed along s and L along z.
//
// While a labelling is being made, L[p] = -1 for background and otherwise the index of a voxel of the same component that is not
// larger than p (a parent link; L[p] == p: a root).  Links only ever decrease (atomicMin), so every loop that follows them ends, and
// no workgroup waits for another: cc_union is lock-free (a failed atomicMin hands back the link it has to follow next), not a spin.
// A load that sees an older link still sees a voxel of the same component with a smaller index, which is all cc_find needs.
//   k_cc_init     foreground test; every voxel links to the start of its z-run inside the tile's 64 pixels (one ballot per row)
//   k_cc_merge    unions with the neighbours of smaller index that the runs and the other voxels' unions do not already imply
//   k_cc_flatten  every voxel links to its root; the roots of every 256 voxels are counted
//   k_cc_scan     exclusive prefix sum of those counts (one workgroup, a fixed order); the total is K
//   k_cc_number   root r, the k-th in index order, takes the code ~(k + 1) (<= -2) and opens record k with first = r
//   k_cc_relabel  background -> 0, every other voxel -> the number of its root; k_cc_roots then writes the K roots' own numbers
// After that L holds 0 for background and 1..K in ascending order of the components' smallest index.  Everything is integer
// arithmetic whose result does not depend on the order in which the atomics arrive.
#pragma once

namespace tomo {

// = tomo_component (include/tomo_hip.h), 72 bytes; a[] = voxels, sum_s, sum_y, sum_z, surface
struct CcRecord { long long a[5]; long long first; int mn[3], mx[3]; };
static_assert(sizeof(CcRecord) == 72, "the record of the header");

__device__ __forceinline__ int cc_find(const int *L, int a)
{
    int b;
    while ((b = __atomic_load_n(&L[a], __ATOMIC_RELAXED)) != a) a = b;     // b < a: ends at a root
    return a;
}

// a and b (both foreground) end up in one tree.  Every round either returns or continues with a strictly smaller a + b.
__device__ __forceinline__ void cc_union(int *L, int a, int b)
{
    for (;;) {
        a = cc_find(L, a); b = cc_find(L, b);
        if (a == b) return;
        if (a > b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(&L[b], a);
        if (old == b) return;            // b was still a root and now links to a
        b = old;                         // b had been linked to `old` meanwhile (L[b] is now min(old, a)): a and old remain to be joined
    }
}

__global__ __launch_bounds__(256) void k_cc_init(const float *__restrict__ x, int *__restrict__ L, float lo, float hi, int n, int npix, int nx, int sx)
{
    __shared__ uint8_t tile[64][65];
    const int p0 = blockIdx.x * 64, s0 = blockIdx.y * 64, c = threadIdx.x & 63, r = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int pix = p0 + 4 * k + r, s = s0 + c;
        bool f = false;
        if (pix < npix && s < nx) { const float v = x[(size_t)pix * sx + s]; f = lo <= v && v <= hi; }   // a NaN fails both
        tile[4 * k + r][c] = f;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int s = s0 + 4 * k + r, pix = p0 + c;           // s is wave-uniform, the lanes are 64 consecutive pixels
        const bool in = s < nx && pix < npix, f = in && tile[c][4 * k + r];
        const uint64_t fg = __ballot(f), rs = __ballot(pix % n == 0);
        // a run starts at lane 0, at the first pixel of an image row and behind a background voxel
        const uint64_t starts = (rs | (~fg << 1) | 1ull) & (~0ull >> (63 - c));
        const int j = 63 - __clzll((long long)starts);
        if (in) L[(size_t)s * npix + pix] = f ? (int)((size_t)s * npix + p0 + j) : -1;
    }
}

// Unions with the 3 (C = 6) or 13 (C = 26) neighbours of smaller index.  Left out are those that follow from others:
//   z - 1: joined by the runs of k_cc_init except across a tile edge (pix a multiple of 64);
//   a face pair (p, q), q = p - N or p - N^2: where p - 1 and q - 1 are foreground too, p ~ p - 1 and q ~ q - 1 (z-neighbours) and
//       (p - 1, q - 1) is the same kind of pair one column to the left (induction on z);
//   an in-plane diagonal: where one of the two voxels between them is foreground (a z-neighbour pair and a face pair);
//   the 8 other voxels of the plane s - 1: where the face neighbour in that plane is foreground (it is a 26-neighbour of all of them
//       in its own plane, and of p by the face pair).
template <int C>
__global__ __launch_bounds__(256) void k_cc_merge(int *__restrict__ L, int n, int npix, int nvox)
{
    static_assert(C == 6 || C == 26, "connectivity");
    const int64_t gp = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (gp >= nvox) return;
    const int p = (int)gp;
    if (L[p] < 0) return;
    const int pix = p % npix, s = p / npix, y = pix / n, z = pix % n;
    const bool zm = z > 0 && L[p - 1] >= 0;
    if (zm && (pix & 63) == 0) cc_union(L, p, p - 1);
    bool ym = false;
    if (y > 0) {
        ym = L[p - n] >= 0;
        if (ym && !(zm && L[p - n - 1] >= 0)) cc_union(L, p, p - n);
        if (C == 26 && !ym) {
            if (z > 0 && !zm && L[p - n - 1] >= 0) cc_union(L, p, p - n - 1);
            if (z + 1 < n && L[p - n + 1] >= 0 && !(L[p + 1] >= 0)) cc_union(L, p, p - n + 1);
        }
    }
    if (s > 0) {
        const int q = p - npix;
        const bool sm = L[q] >= 0;
        if (sm) {
            if (!(zm && L[q - 1] >= 0)) cc_union(L, p, q);
        } else if (C == 26) {
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
                for (int dz = -1; dz <= 1; ++dz) {
                    if (!dy && !dz) continue;
                    if (y + dy < 0 || y + dy >= n || z + dz < 0 || z + dz >= n) continue;
                    const int w = q + dy * n + dz;
                    if (L[w] >= 0) cc_union(L, p, w);
                }
            }
        }
    }
}

// the number of set flags among the workgroup's threads before this one (thread order), and the workgroup's total
__device__ __forceinline__ int cc_block_rank(bool flag, int &total)
{
    __shared__ int wsum[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint64_t m = __ballot(flag);
    if (lane == 0) wsum[w] = __popcll(m);
    __syncthreads();
    int before = __popcll(m & ((1ull << lane) - 1ull));
    total = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) { before += k < w ? wsum[k] : 0; total += wsum[k]; }
    return before;
}

__global__ __launch_bounds__(256) void k_cc_flatten(int *__restrict__ L, int *__restrict__ counts, int nvox)
{
    const int64_t gp = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool root = false;
    if (gp < nvox) {
        const int p = (int)gp, v = L[p];
        if (v >= 0) {
            const int r = cc_find(L, v);
            if (r != v) __atomic_store_n(&L[p], r, __ATOMIC_RELAXED);
            root = r == p;
        }
    }
    int total;
    cc_block_rank(root, total);
    if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

// counts[0 .. nblk) -> their exclusive prefix sums, counts[nblk] = the total.  One workgroup walks the array in pieces of 1024.
__global__ __launch_bounds__(1024) void k_cc_scan(int *__restrict__ counts, int nblk)
{
    __shared__ int wsum[16];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int carry = 0;
    for (int base = 0; base < nblk; base += 1024) {
        const int i = base + (int)threadIdx.x;
        const int v = i < nblk ? counts[i] : 0;
        int incl = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(incl, d); if (lane >= d) incl += t; }
        if (lane == 63) wsum[w] = incl;
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int k = 0; k < 16; ++k) { before += k < w ? wsum[k] : 0; total += wsum[k]; }
        if (i < nblk) counts[i] = carry + before + incl - v;
        carry += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) counts[nblk] = carry;
}

__global__ __launch_bounds__(256) void k_cc_number(int *__restrict__ L, const int *__restrict__ offs, CcRecord *__restrict__ rec, int nvox)
{
    const int64_t gp = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool root = gp < nvox && L[gp] == (int)gp;
    int total;
    const int k = offs[blockIdx.x] + cc_block_rank(root, total);
    if (!root) return;
    L[gp] = ~(k + 1);
    CcRecord r;
#pragma unroll
    for (int i = 0; i < 5; ++i) r.a[i] = 0;
    r.first = gp;
#pragma unroll
    for (int i = 0; i < 3; ++i) { r.mn[i] = 0x7fffffff; r.mx[i] = -1; }
    rec[k] = r;
}

__global__ __launch_bounds__(256) void k_cc_relabel(int *__restrict__ L, int nvox)
{
    const int64_t gp = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (gp >= nvox) return;
    const int v = L[gp];
    if (v == -1) L[gp] = 0;
    else if (v >= 0) L[gp] = ~L[v];      // v is a root: its code stands until k_cc_roots
}

__global__ __launch_bounds__(256) void k_cc_roots(int *__restrict__ L, const CcRecord *__restrict__ rec, int K)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k < K) L[rec[k].first] = (int)k + 1;
}

// sum of the positions of the set bits of m
__device__ __forceinline__ int cc_bit_positions(uint64_t m)
{
    return __popcll(m & 0xaaaaaaaaaaaaaaaaull) + 2 * __popcll(m & 0xccccccccccccccccull) + 4 * __popcll(m & 0xf0f0f0f0f0f0f0f0ull) +
           8 * __popcll(m & 0xff00ff00ff00ff00ull) + 16 * __popcll(m & 0xffff0000ffff0000ull) + 32 * __popcll(m & 0xffffffff00000000ull);
}

// ---- k_cc_stats: the measurements, from the finished labels ---------------------------------------------------------------------
// A wave owns 64 consecutive z of `yb` rows of one slice.  In a row s and y are wave-uniform, so what the lanes of one label add to its
// record follows from the ballot of those lanes alone (count, sum and extremes of their z: bit counts), without a cross-lane sum.
// The wave carries the sums of ONE label in scalars from row to row and sends them (11 integer atomics by lane 0) only when another
// label turns up or its rows end: a component that fills the wave's rows costs one set of atomics per wave, not per row.
__global__ __launch_bounds__(256) void k_cc_stats(const int *__restrict__ L, CcRecord *__restrict__ rec, int n, int nx, int yb)
{
    const int lane = threadIdx.x & 63;
    const int nzc = (n + 63) / 64, nyb = (n + yb - 1) / yb;
    const int64_t item = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (item >= (int64_t)nx * nyb * nzc) return;
    const int z0 = (int)(item % nzc) * 64, y0 = (int)((item / nzc) % nyb) * yb, s = (int)(item / ((int64_t)nzc * nyb));
    const int y1 = min(y0 + yb, n), z = z0 + lane, npix = n * n;
    int ak = 0, amn_y = 0, amx_y = 0, amn_z = 0, amx_z = 0;
    long long avox = 0, asy = 0, asz = 0, asurf = 0;
    auto flush = [&]() __attribute__((always_inline)) {
        if (ak > 0 && lane == 0) {
            CcRecord *r = rec + (ak - 1);
            atomicAdd((unsigned long long *)&r->a[0], (unsigned long long)avox);
            atomicAdd((unsigned long long *)&r->a[1], (unsigned long long)(avox * s));
            atomicAdd((unsigned long long *)&r->a[2], (unsigned long long)asy);
            atomicAdd((unsigned long long *)&r->a[3], (unsigned long long)asz);
            atomicAdd((unsigned long long *)&r->a[4], (unsigned long long)asurf);
            atomicMin(&r->mn[0], s); atomicMin(&r->mn[1], amn_y); atomicMin(&r->mn[2], amn_z);
            atomicMax(&r->mx[0], s); atomicMax(&r->mx[1], amx_y); atomicMax(&r->mx[2], amx_z);
        }
    };
    for (int y = y0; y < y1; ++y) {
        const int64_t p = ((int64_t)s * n + y) * n + z;
        const int k = z < n ? L[p] : 0;
        bool surf = false;
        if (k > 0)
            surf = z == 0 || z == n - 1 || y == 0 || y == n - 1 || s == 0 || s == nx - 1 || L[p - 1] == 0 || L[p + 1] == 0 || L[p - n] == 0 ||
                   L[p + n] == 0 || L[p - npix] == 0 || L[p + npix] == 0;
        uint64_t rem = __ballot(k > 0);
        while (rem) {
            const int kk = __shfl(k, __ffsll((long long)rem) - 1);
            const uint64_t m = __ballot(k == kk), ms = __ballot(k == kk && surf);
            const int cnt = __popcll(m), lo = z0 + __ffsll((long long)m) - 1, hi = z0 + 63 - __clzll((long long)m);
            if (kk != ak) { flush(); ak = kk; avox = asy = asz = asurf = 0; amn_y = y; amn_z = lo; amx_z = hi; }
            avox += cnt; asy += (long long)cnt * y; asz += (long long)cnt * z0 + cc_bit_positions(m); asurf += __popcll(ms);
            amx_y = y; amn_z = min(amn_z, lo); amx_z = max(amx_z, hi);
            rem &= ~m;
        }
    }
    flush();
}

// ---- k_cc_keep: x(v) = fill where label(v) > 0 and keep[label(v)] == 0; no other voxel is written ---------------------------------
__global__ __launch_bounds__(256) void k_cc_keep(float *__restrict__ x, const int *__restrict__ L, const uint8_t *__restrict__ keep, float fill,
                                                 int npix, int nx, int sx)
{
    __shared__ uint8_t tile[64][65];
    const int p0 = blockIdx.x * 64, s0 = blockIdx.y * 64, c = threadIdx.x & 63, r = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int s = s0 + 4 * k + r, pix = p0 + c;
        bool drop = false;
        if (s < nx && pix < npix) { const int l = L[(size_t)s * npix + pix]; drop = l > 0 && !keep[l]; }
        tile[c][4 * k + r] = drop;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int pix = p0 + 4 * k + r, s = s0 + c;
        if (pix < npix && s < nx && tile[4 * k + r][c]) x[(size_t)pix * sx + s] = fill;
    }
}

}  // namespace tomo
