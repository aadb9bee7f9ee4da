/*
 * ppp_removal.h -- predicted material removal per cloud point (ppp_get_path_removal): the balls of
 * the path contacts, each weighted by where the point lies inside it and by the path length its sample stands for.  Reads the
 * sample table of k_pcon_offsets / k_pcon_samples (ppp_contact.h) as those kernels leave it; every sum here has one fixed
 * order, so map and statistics are the same bits in every run.  No float atomics.
 */
#pragma once
#include "ppp_contact.h"

/* the length of the segment between two samples: double differences of the float positions, ((dx*dx) + dy*dy) + dz*dz, one
   rounding per operation (the unit is built without contraction); 0 where an end is not finite (B.43) */
__device__ inline double prem_seg(const float4 &a, const float4 &b)
{
    const float big = 3.402823466e+38f;
    if (!(fabsf(a.x) <= big && fabsf(a.y) <= big && fabsf(a.z) <= big && fabsf(b.x) <= big && fabsf(b.y) <= big && fabsf(b.z) <= big)) return 0.0;
    const double dx = (double)b.x - (double)a.x, dy = (double)b.y - (double)a.y, dz = (double)b.z - (double)a.z;
    return sqrt(((dx * dx) + dy * dy) + dz * dz);
}

/* Workgroup i = slice i of the table, one thread per sample: ds[row] = half the segment before the sample plus half the one
   after it, within the slice's rows [off[i], off[i + 1]) -- an end sample has one segment, a lone sample none (a segment is
   >= +0, so 0.5 * (before + after) is 0.5 * the one segment where the other is missing, bit for bit).  A sample whose radius
   is NaN still has its position.  slice_len[i] = the slice's ds added in sample order by one thread (a few hundred terms,
   staged in LDS PCON_T at a time): the host adds the slices in order to the path length. */
__global__ void __launch_bounds__(PCON_T) k_prem_ds(const float4 *__restrict__ tab, const int *__restrict__ off, double *__restrict__ ds,
        double *__restrict__ slice_len)
{
    __shared__ double s_ds[PCON_T];
    const int i = blockIdx.x, o0 = off[i], m = off[i + 1] - o0;
    double len = 0.0; /* thread 0's */
    for (int base = 0; base < m; base += PCON_T) { /* (m is the workgroup's: every thread meets the barriers) */
        const int j = base + threadIdx.x;
        double d = 0.0;
        if (j < m) {
            const float4 q = tab[o0 + j];
            const double before = j > 0 ? prem_seg(tab[o0 + j - 1], q) : 0.0;
            const double after = j + 1 < m ? prem_seg(q, tab[o0 + j + 1]) : 0.0;
            d = 0.5 * (before + after);
            ds[o0 + j] = d;
        }
        s_ds[threadIdx.x] = d;
        __syncthreads();
        if (threadIdx.x == 0) {
            const int c = min(PCON_T, m - base);
            for (int t = 0; t < c; ++t) len += s_ds[t];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) slice_len[i] = len;
}

/* the weight of a held point at squared distance d2 inside a ball of squared radius r2 (d2 <= r2, so u <= 1), B.44 */
template <int PROFILE>
__device__ inline double prem_weight(float d2, float r2)
{
    if (PROFILE == PPP_REMOVAL_FLAT) return 1.0;
    const double u = r2 == 0.f ? 0.0 : (double)d2 / (double)r2;
    return PROFILE == PPP_REMOVAL_PARABOLIC ? 1.0 - u : sqrt(1.0 - u);
}

/* The removal map by the point walk (pcon_walk_points, ppp_contact.h): a sum in place of k_pcon_points's count.  The walk hands
   over a point's held pairs in ascending (slice, sample) order (see there), so the one double accumulator adds w * ds in that
   order and the sum is the same in every run.  The profile is a template parameter: the inner loop has no branch on it; the
   division and the square root are paid per held pair, not per candidate.  One 8-byte store at the point's cloud index, and
   held[index] = 1 (a held point's sum may be 0: a rim point, a lone sample); points that no ball holds keep the zeros of the
   memsets. */
struct PremAcc { double sum = 0.0; bool hit = false; };
template <int PROFILE>
__global__ void __launch_bounds__(PCON_T) k_prem_points(const DevMeta *m, const float4 *__restrict__ sorted4, const float4 *__restrict__ tab,
        const double *__restrict__ ds, const int *__restrict__ off, const unsigned *__restrict__ reach, int nsl, double *__restrict__ removal,
        unsigned char *__restrict__ held)
{
    pcon_walk_points<PremAcc>(m, sorted4, tab, off, reach, nsl,
        [&](PremAcc &a, int, int j, float d2, float r2) { a.hit = true; a.sum += prem_weight<PROFILE>(d2, r2) * ds[j]; },
        [&](const PremAcc &a, const float4 &p) { if (a.hit) { const int id = idx_of(p); removal[id] = a.sum; held[id] = 1; } });
}

/* The accumulators of the removal statistics: [0] touched, [1] the largest removal of a touched point as its bit pattern (a
   removal is >= +0, and such doubles order as their bits do), [2] the complement of the smallest one's (so a maximum finds
   it; 0 = no touched point), [3 .. 66] the bins, [67] the refusal word of the sample kernels. */
#define PREM_ACC_BINS 3
#define PREM_ACC_ERR (PREM_ACC_BINS + PPP_CONTACT_BINS)
#define PREM_ACC_WORDS (PREM_ACC_ERR + 1)

/* first phase: touched, the largest and the smallest removal over the held points -- integer atomics on the keys, a wave, a
   workgroup, then one per workgroup, as k_pcon_stats counts */
__global__ void __launch_bounds__(PCON_T) k_prem_range(const double *__restrict__ removal, const unsigned char *__restrict__ held, int n,
        unsigned long long *__restrict__ acc)
{
    __shared__ unsigned long long s_a[3];
    if (threadIdx.x < 3) s_a[threadIdx.x] = 0;
    __syncthreads();
    unsigned long long cnt = 0, hi = 0, nlo = 0;
    for (int i = blockIdx.x * PCON_T + threadIdx.x; i < n; i += gridDim.x * PCON_T) {
        if (!held[i]) continue;
        const unsigned long long k = (unsigned long long)__double_as_longlong(removal[i]);
        ++cnt; hi = max(hi, k); nlo = max(nlo, ~k);
    }
    cnt = wave_sum(cnt); hi = wave_max_bits(hi); nlo = wave_max_bits(nlo);
    if ((threadIdx.x & 63) == 0 && cnt) { atomicAdd(&s_a[0], cnt); atomicMax(&s_a[1], hi); atomicMax(&s_a[2], nlo); }
    __syncthreads();
    if (threadIdx.x == 0 && s_a[0]) { atomicAdd(acc, s_a[0]); atomicMax(acc + 1, s_a[1]); atomicMax(acc + 2, s_a[2]); }
}

/* second phase, behind the first: the histogram against the maximum (range[1]; min(63, floor(removal / max * 63)) in double,
   everything in bin 0 when the maximum is 0) with per-workgroup LDS bins and one integer atomic per non-empty bin, and the
   sums as k_field_stats adds them: workgroup g takes the contiguous part [g per, (g + 1) per) of the map, every thread its
   strided share in index order, block_tree_sum over the threads, psum[g] / psq[g] for the host to add in order. */
__global__ void __launch_bounds__(PCON_T) k_prem_stats(const double *__restrict__ removal, const unsigned char *__restrict__ held, int n, int per,
        const unsigned long long *range, unsigned long long *bins, double *__restrict__ psum, double *__restrict__ psq)
{
    __shared__ int s_bin[PPP_CONTACT_BINS];
    __shared__ double s_sum[PCON_T], s_sq[PCON_T];
    if (threadIdx.x < PPP_CONTACT_BINS) s_bin[threadIdx.x] = 0;
    __syncthreads();
    const double mx = __longlong_as_double((long long)range[1]);
    const int i0 = blockIdx.x * per, i1 = min(n, i0 + per);
    double sum = 0.0, sq = 0.0;
    for (int i = i0 + threadIdx.x; i < i1; i += PCON_T) {
        if (!held[i]) continue;
        const double r = removal[i];
        sum += r; sq += r * r;
        int bin = 0;
        if (mx > 0.0) { bin = (int)floor(r / mx * (double)(PPP_CONTACT_BINS - 1)); bin = bin > PPP_CONTACT_BINS - 1 ? PPP_CONTACT_BINS - 1 : bin; }
        atomicAdd(&s_bin[bin], 1);
    }
    block_tree_sum(s_sum, sum, s_sq, sq);
    if (threadIdx.x < PPP_CONTACT_BINS && s_bin[threadIdx.x]) atomicAdd(bins + threadIdx.x, (unsigned long long)s_bin[threadIdx.x]);
    if (threadIdx.x == 0) { psum[blockIdx.x] = s_sum[0]; psq[blockIdx.x] = s_sq[0]; }
}
