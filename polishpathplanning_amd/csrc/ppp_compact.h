/*
 * ppp_compact.h -- ordered compaction on the device: the cloud filters' survivors (ppp_preproc.h), a slice-range handle's part
 * of the cloud (make_plan), the regions' selected points and heads (ppp_regions.h).  The host side is compact() of ppp_handle.h.
 * k_compact_count and k_compact_emit are instantiated per selector by the unit that owns the selector.
 */
#pragma once
#include "ppp_kernels.h"

/* ------------------------------------------------------------------------------------------------------------------ */
/* Ordered compaction (the points SOR keeps, the voxel heads, MLS's survivors, a range part): per block of            */
/* COMPACT_CHUNK elements the number kept (k_compact_count), the scan of those counts (k_compact_scan), then every    */
/* block writes its kept elements in input order behind its offset (k_compact_emit).  A selector says what is kept:   */
/* begin() loads its per-workgroup constants, load(i) reads element i, keep(i, v) tests it, emit(i, k, v) writes      */
/* the kept element i to slot k from the same v.                                                                      */
/* ------------------------------------------------------------------------------------------------------------------ */
#define COMPACT_CHUNK 1024
template <class Sel>
__global__ void __launch_bounds__(256) k_compact_count(Sel sel, int n, int *block_cnt)
{
    __shared__ int s_c[4];
    sel.begin();
    int c = 0;
    for (int i = blockIdx.x * COMPACT_CHUNK + threadIdx.x; i < min(n, (blockIdx.x + 1) * COMPACT_CHUNK); i += blockDim.x) c += sel.keep(i, sel.load(i));
    c = wave_sum(c);
    if ((threadIdx.x & 63) == 0) s_c[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) block_cnt[blockIdx.x] = s_c[0] + s_c[1] + s_c[2] + s_c[3];
}

/* block counts -> block offsets; the kept total to *total.  Every unit's compactions launch it; it is compiled in the engine's */
#ifdef PPP_KERNELS_FOREIGN
__global__ void k_compact_scan(int *block_cnt, int nblocks, int *total);
#else
__global__ void __launch_bounds__(1024) k_compact_scan(int *block_cnt, int nblocks, int *total)
{
    __shared__ int s_scr[17];
    __shared__ int s_run;
    if (threadIdx.x == 0) s_run = 0;
    __syncthreads();
    for (int base = 0; base < nblocks; base += blockDim.x) {
        const int i = base + threadIdx.x;
        const int c = i < nblocks ? block_cnt[i] : 0;
        int tot;
        const int pre = block_exscan(c, s_scr, &tot);
        const int run = s_run;
        if (i < nblocks) block_cnt[i] = run + pre;
        __syncthreads();
        if (threadIdx.x == 0) s_run = run + tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = s_run;
}
#endif

template <class Sel>
__global__ void __launch_bounds__(256) k_compact_emit(Sel sel, int n, const int *__restrict__ block_off)
{
    __shared__ int s_scr[17];
    __shared__ int s_run;
    sel.begin();
    if (threadIdx.x == 0) s_run = block_off[blockIdx.x];
    __syncthreads();
    const int i0 = blockIdx.x * COMPACT_CHUNK, i1 = min(n, i0 + COMPACT_CHUNK);
    for (int base = i0; base < i1; base += blockDim.x) {
        const int i = base + threadIdx.x;
        typename Sel::Val v{};
        int keep = 0;
        if (i < i1) { v = sel.load(i); keep = sel.keep(i, v); }
        int tot;
        const int pre = block_exscan(keep, s_scr, &tot);
        const int run = s_run;
        if (keep) sel.emit(i, run + pre, v);
        __syncthreads();
        if (threadIdx.x == 0) s_run = run + tot;
        __syncthreads();
    }
}

/* ------------------------------------------------------------------ */
/* Slice-range handles (SURVEY.md 8e case ii): the points of the cloud   */
/* whose x lies in [lo, hi] -- the interval a handle indexes --, in the  */
/* cloud's own order (ties on the cloud index break as in the whole      */
/* cloud), with their cloud indices.  Built once per plan; the hot path  */
/* then streams the part only.                                           */
/* ------------------------------------------------------------------ */
struct PartSel {
    using Val = float;
    const float *X, *Y, *Z;
    float lo, hi;
    float *X2, *Y2, *Z2;
    int *idx2;
    __device__ void begin() {}
    __device__ float load(int i) const { return X[i]; }
    __device__ bool keep(int, float x) const { return x >= lo && x <= hi; } /* NaN (a dropped point) fails both */
    __device__ void emit(int i, int k, float x) const { const float y = Y[i], z = Z[i]; X2[k] = x; Y2[k] = y; Z2[k] = z; idx2[k] = i; }
};
