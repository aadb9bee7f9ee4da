/*
 * ppp_dwell.h -- the dwell schedule (ppp_get_path_dwell): a factor per row of the sample table that
 * steers the predicted removal of ppp_removal.h towards a target map.  The forward pass is k_prem_points itself on the scaled
 * lengths; the kernels here scale, take the ratio per point, walk every ball for the transposed sums (k_dwell_back, in fixed
 * point: integer sums have no order), clamp, and reduce the residual and the factors' statistics.  No float atomics, no float
 * sum whose order is not fixed.
 */
#pragma once
#include "ppp_removal.h"

#define DWELL_FIXED 268435456.0 /* F = 2^28 */
#define DWELL_G_MAX 64.0        /* the ratio's clamp: [2^-6, 2^6] */

/* dst[j] = ds[j] * t[j], one rounding: the lengths the forward pass weighs with */
__global__ void __launch_bounds__(PCON_T) k_dwell_scale(const double *__restrict__ ds, const double *__restrict__ t, int rows, double *__restrict__ dst)
{
    const int j = blockIdx.x * PCON_T + threadIdx.x;
    if (j < rows) dst[j] = ds[j] * t[j];
}

/* One thread per cloud index: g[i] = T_i / R_i clamped to [2^-6, 2^6] for a held point with R_i > 0, 1 for a held point with
   R_i == 0; target == nullptr: T_i = level.  Points that no ball holds are never read and keep the zeros of the memset. */
__global__ void __launch_bounds__(PCON_T) k_dwell_ratio(const double *__restrict__ removal, const double *__restrict__ target, double level,
        const unsigned char *__restrict__ held, int n, double *__restrict__ g)
{
    const int i = blockIdx.x * PCON_T + threadIdx.x;
    if (i >= n || !held[i]) return;
    const double r = removal[i], tg = target ? target[i] : level;
    g[i] = r > 0.0 ? fmin(fmax(tg / r, 1.0 / DWELL_G_MAX), DWELL_G_MAX) : 1.0;
}

/* the y-windows of 64 neighbouring slabs: exclusive prefix of their sizes and their first positions -- what the ball walk
   (wave_ball_candidates, ppp_contact.h) uses of a wave's LDS block */
struct DwellWaveLds { int off[64], w0[64]; };

/* The transposed walk of one ball, all 64 lanes together: num = the sum over the held points i of llrint((a_ij * g_i) * F),
   den = the sum of llrint(a_ij * F) (den only where WITH_DEN), a_ij = prem_weight<PROFILE>(d2, r2), held = dist2_flann <= r2
   -- k_prem_points's pairs.  The candidates are wave_ball_candidates's, the very ones wave_mark_ball tests; every lane adds the
   integers of the candidates it tests, then one wave reduction: every lane returns the ball's sums.  The walk visits a point
   once, so a pair is added once. */
template <int PROFILE, bool WITH_DEN>
__device__ inline void wave_ball_sums(const SlabView &V, const DynGrid &G, DwellWaveLds &L, float qx, float qy, float qz, float r, float r2,
                                      const double *__restrict__ g, long long &num, long long &den)
{
    long long sn = 0, sd = 0;
    wave_ball_candidates(V, G, L, qx, qy, r, [&](const float4 &c) {
        const float d2 = dist2_flann(qx, qy, qz, c.x, c.y, c.z);
        if (d2 <= r2) {
            const double w = prem_weight<PROFILE>(d2, r2);
            sn += llrint((w * g[idx_of(c)]) * DWELL_FIXED);
            if (WITH_DEN) sd += llrint(w * DWELL_FIXED);
        }
    });
    num = wave_sum(sn);
    den = WITH_DEN ? wave_sum(sd) : 0;
}

/* One wave per row of the sample table (DYN_WAVES rows a workgroup): the row's ball (position and r2 as k_pcon_samples left
   them, r = sqrtf(r2)) walked by wave_ball_sums, one store per row.  A row whose r2 or position is NaN holds nothing: 0.  den
   does not change between the iterations: the first launch (WITH_DEN) writes it, the later ones leave it alone. */
template <int PROFILE, bool WITH_DEN>
__global__ void __launch_bounds__(64 * DYN_WAVES) k_dwell_back(ContactIndex I, const float4 *__restrict__ tab, int rows, const double *__restrict__ g,
        long long *__restrict__ num, long long *__restrict__ den)
{
    __shared__ DwellWaveLds s_w[DYN_WAVES];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int j = blockIdx.x * DYN_WAVES + wv;
    if (j >= rows) return; /* (the whole wave; the routine below has wave barriers only) */
    const DynGrid G = dyn_grid(I.m);
    const float4 q = tab[j];
    long long sn = 0, sd = 0;
    if (q.w == q.w && q.x == q.x && q.y == q.y && q.z == q.z)
        wave_ball_sums<PROFILE, WITH_DEN>(I.view(), G, s_w[wv], q.x, q.y, q.z, sqrtf(q.w), q.w, g, sn, sd);
    if (lane == 0) { num[j] = sn; if (WITH_DEN) den[j] = sd; }
}

/* t[j] = min(max(t[j] * (num[j] / den[j]), dmin), dmax) where den[j] > 0; a row that holds nothing keeps its factor */
__global__ void __launch_bounds__(PCON_T) k_dwell_update(const long long *__restrict__ num, const long long *__restrict__ den, int rows, double dmin,
        double dmax, double *__restrict__ t)
{
    const int j = blockIdx.x * PCON_T + threadIdx.x;
    if (j >= rows || den[j] <= 0) return;
    t[j] = fmin(fmax(t[j] * ((double)num[j] / (double)den[j]), dmin), dmax);
}

/* The factors' statistics over the rows with den > 0: acc[0] rows at dmin, acc[1] rows at dmax, acc[2] the largest factor as its
   bit pattern (a factor is > 0: such doubles order as their bits do), acc[3] the complement of the smallest one's (0: no such
   row) -- integer atomics, a wave, then one per wave that has something */
__global__ void __launch_bounds__(PCON_T) k_dwell_stats(const double *__restrict__ t, const long long *__restrict__ den, int rows, double dmin, double dmax,
        unsigned long long *__restrict__ acc)
{
    unsigned long long lo = 0, hi = 0, mx = 0, nmn = 0;
    for (int j = blockIdx.x * PCON_T + threadIdx.x; j < rows; j += gridDim.x * PCON_T) {
        if (den[j] <= 0) continue;
        const double v = t[j];
        const unsigned long long k = (unsigned long long)__double_as_longlong(v);
        lo += v == dmin; hi += v == dmax; mx = max(mx, k); nmn = max(nmn, ~k);
    }
    lo = wave_sum(lo); hi = wave_sum(hi); mx = wave_max_bits(mx); nmn = wave_max_bits(nmn);
    if ((threadIdx.x & 63) == 0 && nmn) { atomicAdd(acc, lo); atomicAdd(acc + 1, hi); atomicMax(acc + 2, mx); atomicMax(acc + 3, nmn); }
}

/* The residual's sum by k_prem_stats's fixed-order scheme: workgroup g takes the contiguous part [g per, (g + 1) per) of the
   map, every thread its strided share in index order, block_tree_sum over the threads, psum[g] for the host to add in order.
   e_i = (R_i - T_i) / level over the held points, the sum of e_i * e_i; target == nullptr: T_i = level. */
__global__ void __launch_bounds__(PCON_T) k_dwell_resid(const double *__restrict__ removal, const double *__restrict__ target, double level,
        const unsigned char *__restrict__ held, int n, int per, double *__restrict__ psum)
{
    __shared__ double s_sum[PCON_T];
    const int i0 = blockIdx.x * per, i1 = min(n, i0 + per);
    double sum = 0.0;
    for (int i = i0 + threadIdx.x; i < i1; i += PCON_T) {
        if (!held[i]) continue;
        const double e = (removal[i] - (target ? target[i] : level)) / level;
        sum += e * e;
    }
    block_tree_sum(s_sum, sum);
    if (threadIdx.x == 0) psum[blockIdx.x] = s_sum[0];
}
