/*
 * ppp_deviation.h -- the deviation map of one handle's cloud against another handle's (ppp_get_deviation, DESIGN.md §7j,
 * B.61-B.66): for every point of the scan its nearest point of the reference cloud, the signed distance along that point's
 * normal, its local mean and the target map the dwell schedule takes.  The search runs the scan's points, in the scan's slab
 * order, through the REFERENCE's slab index: the one kernel of the engine that reads two handles.  Minima over (distance, index),
 * integer sums and fixed-order double sums only: maps and statistics are the same bits in every run.  No float atomics.
 */
#pragma once
#include "ppp_contact.h"

#define DEV_T 256
#define DEV_FIXED 16777216.0 /* 2^24: a deviation in fixed point (B.63) */

/* the quiet NaN every map holds where it holds no number: one bit pattern, so maps compare as bytes */
__device__ inline double dev_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

/* a double as an unsigned that orders like it (-0 below +0, NaN aside); 0 is below every key of a number: "none" */
__host__ __device__ inline unsigned long long ordered_key64(double d)
{
    unsigned long long u; __builtin_memcpy(&u, &d, 8);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__host__ __device__ inline double ordered_unkey64(unsigned long long k)
{
    k = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    double d; __builtin_memcpy(&d, &k, 8);
    return d;
}

/* The nearest indexed point of V within bound2 (<=: a point at exactly bound2 is found; INFINITY = no limit) in the slabs
   [b0, b1) of V -- the slabs the searched handle sorted --, ties to the lower cloud index; -1 when there is none.
   nearest_in_slabs's walk, started at the bound instead of at infinity -- a slab farther in x than the bound closes its side
   at once, so a query outside the reference costs its own slab's y window and nothing else -- and entered through the slabs'
   y-bucket rows.  The slab of the query may lie outside [b0, b1): it is then empty, and either walk starts at the nearer end
   of the interval.  WHOLE: the whole index, b0 and b1 are not read.  slab_of clamps into [0, B), so with b0 = 0, b1 = B the
   query's slab is always inside and the walks start at max(b + 1, 0) = b + 1 and min(b - 1, B - 1) = b - 1: WHOLE writes
   those bounds at compile time, and the whole-index kernels keep the instructions they had.  *found: the point, *d2: its
   distance. */
template <bool WHOLE>
__device__ inline int dev_nearest_within(const SlabView &V, int b0, int b1, float qx, float qy, float qz, float bound2, float4 *found,
                                         float *d2)
{
    if (WHOLE) { b0 = 0; b1 = V.m->B; }
    float best = bound2;
    int bidx = 0x7fffffff;
    float4 bp = make_float4(NAN, NAN, NAN, 0.f);
    auto visit = [&](const float4 &c) {
        const float dy = qy - c.y;
        if (dy * dy > best) return false;
        const float d = dist2_flann(qx, qy, qz, c.x, c.y, c.z);
        const int id = idx_of(c);
        if (d < best || (d == best && id < bidx)) { best = d; bidx = id; bp = c; }
        return true;
    };
    auto scan_slab = [&](int bb, int s0, int s1) {
        int lo, hi;
        V.narrow(bb, s0, s1, qy, lo, hi);
        const int p = lower_bound_y(V, lo, hi, qy);
        for (int i = p; i < s1; ++i) if (!visit(V.sorted4[i])) break;
        for (int i = p - 1; i >= s0; --i) if (!visit(V.sorted4[i])) break;
    };
    const int b = slab_of(V.m, qx);
    if (WHOLE || (b >= b0 && b < b1)) {
        const int s0 = V.slab_start[b], s1 = V.slab_start[b + 1];
        if (s0 < s1) scan_slab(b, s0, s1);
    }
    for (int bb = WHOLE ? b + 1 : max(b + 1, b0); bb < b1; ++bb) {
        const int s0 = V.slab_start[bb], s1 = V.slab_start[bb + 1];
        if (s0 >= s1) continue;
        const float dx = V.slab_xmin[bb] - qx;
        if (dx > 0.f && dx * dx > best) break;
        scan_slab(bb, s0, s1);
    }
    for (int bb = WHOLE ? b - 1 : min(b - 1, b1 - 1); bb >= b0; --bb) {
        const int s0 = V.slab_start[bb], s1 = V.slab_start[bb + 1];
        if (s0 >= s1) continue;
        const float dx = qx - V.slab_xmax[bb];
        if (dx > 0.f && dx * dx > best) break;
        scan_slab(bb, s0, s1);
    }
    *found = bp; *d2 = best;
    return bidx == 0x7fffffff ? -1 : bidx;
}

/* The pair rule of every scan-against-reference kernel: the partner of the query (qx, qy, qz) is the nearest point of the
   reference's index R within md2 in its slabs [b0, b1), or in all of it (WHOLE; dev_nearest_within); PPP_DEV_TOO_FAR where there is none or the
   reference indexes nothing (nref == 0), PPP_DEV_NO_NORMAL where its normal has a NaN in any of its four components, else
   PPP_DEV_MATCHED.  j: the partner's cloud index (-1: none), q: the partner, d2: its distance, n: its normal. */
struct DevPair {
    int j;
    float d2;
    float4 q, n;
};
template <bool WHOLE>
__device__ __attribute__((always_inline)) inline int dev_pair(const ContactIndex &R, int nref, int b0, int b1, float qx, float qy, float qz,
                                                              float md2, DevPair &P)
{
    P.q = make_float4(NAN, NAN, NAN, 0.f);
    P.d2 = NAN;
    P.j = nref > 0 ? dev_nearest_within<WHOLE>(R.view(), b0, b1, qx, qy, qz, md2, &P.q, &P.d2) : -1;
    if (P.j < 0) return PPP_DEV_TOO_FAR;
    P.n = R.normals4[P.j];
    if (!(P.n.x == P.n.x && P.n.y == P.n.y && P.n.z == P.n.z && P.n.w == P.n.w)) return PPP_DEV_NO_NORMAL;
    return PPP_DEV_MATCHED;
}

/* The entries of the maps that the query p (cloud index id) owns, from dev_pair's result st, P: status, ref_index where a
   partner was found, and for a matched point d2, the deviation -- the double differences of the floats against the reference's
   normal, ((ex*nx) + ey*ny) + ez*nz, one rounding per operation -- and its fixed-point term. */
__device__ __attribute__((always_inline)) inline void dev_entry(const float4 &p, int id, int st, const DevPair &P, double *__restrict__ dev,
        long long *__restrict__ fix, float *__restrict__ d2, int *__restrict__ ref_index, unsigned char *__restrict__ status)
{
    status[id] = (unsigned char)st;
    if (st == PPP_DEV_TOO_FAR) return;
    ref_index[id] = P.j;
    if (st != PPP_DEV_MATCHED) return;
    const double ex = (double)p.x - (double)P.q.x, ey = (double)p.y - (double)P.q.y, ez = (double)p.z - (double)P.q.z;
    const double v = ((ex * (double)P.n.x) + ey * (double)P.n.y) + ez * (double)P.n.z;
    dev[id] = v; d2[id] = P.d2; fix[id] = llrint(v * DEV_FIXED);
}

/* The hot path: a thread per indexed point of the scan, in the scan's slab order (q4 = its sorted4, nq = its n_sorted), so the
   lanes of a wave read neighbouring queries with one coalesced load and search nearly the same windows of the reference's index
   R (its own meta block, slab grid and y-bucket table).  Every thread owns its point's entries of the maps (dev_entry).  The
   maps hold DROPPED / -1 before the launch: points outside the scan's index (non-finite ones) keep that. */
__global__ void __launch_bounds__(DEV_T) k_dev_nearest(const float4 *__restrict__ q4, int nq, const ContactIndex R, int nref, float md2,
        double *__restrict__ dev, long long *__restrict__ fix, float *__restrict__ d2, int *__restrict__ ref_index,
        unsigned char *__restrict__ status)
{
    const int t = blockIdx.x * DEV_T + threadIdx.x;
    if (t >= nq) return;
    const float4 p = q4[t];
    DevPair P;
    const int st = dev_pair<true>(R, nref, 0, 0, p.x, p.y, p.z, md2, P);
    dev_entry(p, idx_of(p), st, P, dev, fix, d2, ref_index, status);
}

/* The local mean (B.63) of the matched point p at position `at` of V's sorted order: the ball of r2 around it in V -- the loop
   of normal_at_indexed_point: its own slab from its own position outwards, the neighbouring slabs of [hb0, hb1) (the slabs the
   handle sorted; 0, V.m->B: all) through their y-bucket rows until one is farther in x than the radius -- with the fixed-point
   terms of the matched points it finds added in a 64-bit integer: no order, the same bits in every run. */
__device__ __attribute__((always_inline)) inline double dev_smooth_at(const SlabView &V, int hb0, int hb1, int at, const float4 &p, float r2,
        const unsigned char *__restrict__ status, const long long *__restrict__ fix)
{
    long long sum = 0;
    int cnt = 0;
    auto scan_from = [&](int s0, int s1, int q0) {
        auto visit = [&](const float4 &c) {
            const float dy = p.y - c.y;
            if (dy * dy > r2) return false;
            const int k = idx_of(c);
            if (dist2_flann(p.x, p.y, p.z, c.x, c.y, c.z) <= r2 && status[k] == PPP_DEV_MATCHED) { sum += fix[k]; ++cnt; }
            return true;
        };
        for (int i = q0; i < s1; ++i) if (!visit(V.sorted4[i])) break;
        for (int i = q0 - 1; i >= s0; --i) if (!visit(V.sorted4[i])) break;
    };
    auto scan_slab = [&](int bb) {
        const int s0 = V.slab_start[bb], s1 = V.slab_start[bb + 1];
        if (s0 >= s1) return;
        if (at >= s0 && at < s1) { scan_from(s0, s1, at); return; } /* the point's own slab: any split inside its window will do */
        int lo, hi;
        V.narrow(bb, s0, s1, p.y, lo, hi);
        scan_from(s0, s1, lower_bound_y(V, lo, hi, p.y));
    };
    const int b = slab_of(V.m, p.x); /* (inside [hb0, hb1): the point is indexed) */
    scan_slab(b);
    for (int bb = b + 1; bb < hb1; ++bb) {
        if (V.slab_start[bb] == V.slab_start[bb + 1]) continue;
        const float dx = V.slab_xmin[bb] - p.x;
        if (dx > 0.f && dx * dx > r2) break;
        scan_slab(bb);
    }
    for (int bb = b - 1; bb >= hb0; --bb) {
        if (V.slab_start[bb] == V.slab_start[bb + 1]) continue;
        const float dx = p.x - V.slab_xmax[bb];
        if (dx > 0.f && dx * dx > r2) break;
        scan_slab(bb);
    }
    return (double)sum / (double)cnt * (1.0 / DEV_FIXED); /* (cnt >= 1: the point itself) */
}

/* a thread per indexed point of the scan, in slab order: a matched point's local mean over the scan's OWN index.  One 8-byte store. */
__global__ void __launch_bounds__(DEV_T) k_dev_smooth(const ContactIndex H, int nq, float r2, const unsigned char *__restrict__ status,
        const long long *__restrict__ fix, double *__restrict__ smoothed)
{
    const int at = blockIdx.x * DEV_T + threadIdx.x;
    if (at >= nq) return;
    const SlabView V = H.view();
    const float4 p = V.sorted4[at];
    const int id = idx_of(p);
    if (status[id] != PPP_DEV_MATCHED) return;
    smoothed[id] = dev_smooth_at(V, 0, V.m->B, at, p, r2, status, fix);
}

/* The accumulators of the deviation statistics: [0 .. 3] points by status, [4] proud, [5] below, [6] the key of -min v, [7] the
   key of max v (ordered_key64; 0 = no matched point), [8] the sum of llrint(v 2^24) as a two's complement word, [9] the key of
   the largest float d2 of a matched point (ordered_key), [10 .. 73] the bins. */
#define DEV_ACC_STATUS 0
#define DEV_ACC_PROUD 4
#define DEV_ACC_BELOW 5
#define DEV_ACC_NMIN 6
#define DEV_ACC_MAX 7
#define DEV_ACC_FIXSUM 8
#define DEV_ACC_D2 9
#define DEV_ACC_BINS 10
#define DEV_ACC_WORDS (DEV_ACC_BINS + PPP_CONTACT_BINS)

/* What a thread of a target kernel gathers and how a workgroup hands it on: the counts by status, and of a matched point x
   (its float distance d2) proud, below, the extrema's keys and the integer sum; then wave, workgroup (s_a: DEV_ACC_BINS words
   of LDS, zero before the first flush), and one integer atomic per workgroup and non-zero word of acc, as k_prem_range counts. */
struct DevTargetAcc {
    unsigned long long cnt[4] = {0, 0, 0, 0}, proud = 0, below = 0, nlo = 0, hi = 0, fsum = 0, kd = 0;
    __device__ __attribute__((always_inline)) void add(double x, double allowance, float d2)
    {
        proud += x > allowance; below += x < 0.0;
        nlo = max(nlo, ordered_key64(-x)); hi = max(hi, ordered_key64(x));
        fsum += (unsigned long long)llrint(x * DEV_FIXED);
        kd = max(kd, (unsigned long long)ordered_key(d2));
    }
    __device__ __attribute__((always_inline)) void flush(unsigned long long *s_a, unsigned long long *__restrict__ acc)
    {
        for (int c = 0; c < 4; ++c) cnt[c] = wave_sum(cnt[c]);
        proud = wave_sum(proud); below = wave_sum(below); fsum = wave_sum(fsum);
        nlo = wave_max_bits(nlo); hi = wave_max_bits(hi); kd = wave_max_bits(kd);
        if ((threadIdx.x & 63) == 0) {
            for (int c = 0; c < 4; ++c) if (cnt[c]) atomicAdd(&s_a[DEV_ACC_STATUS + c], cnt[c]);
            if (cnt[0]) {
                atomicAdd(&s_a[DEV_ACC_PROUD], proud); atomicAdd(&s_a[DEV_ACC_BELOW], below); atomicAdd(&s_a[DEV_ACC_FIXSUM], fsum);
                atomicMax(&s_a[DEV_ACC_NMIN], nlo); atomicMax(&s_a[DEV_ACC_MAX], hi); atomicMax(&s_a[DEV_ACC_D2], kd);
            }
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int c = 0; c < 6; ++c) if (s_a[c]) atomicAdd(acc + c, s_a[c]);
            if (s_a[DEV_ACC_STATUS]) {
                atomicAdd(acc + DEV_ACC_FIXSUM, s_a[DEV_ACC_FIXSUM]);
                atomicMax(acc + DEV_ACC_NMIN, s_a[DEV_ACC_NMIN]); atomicMax(acc + DEV_ACC_MAX, s_a[DEV_ACC_MAX]); atomicMax(acc + DEV_ACC_D2, s_a[DEV_ACC_D2]);
            }
        }
    }
};

/* The target and the first phase of the statistics, a thread per cloud index: target = gain (v - allowance) where that
   difference is > 0, +0 everywhere else (B.64); a point that is not matched gets the NaN into deviation and v (without
   smoothing v IS deviation: the two are not restrict).  The statistics go through DevTargetAcc. */
__global__ void __launch_bounds__(DEV_T) k_dev_target(const unsigned char *__restrict__ status, double *deviation, double *v,
        const float *__restrict__ d2, int n, double allowance, double gain, double *__restrict__ target, unsigned long long *__restrict__ acc)
{
    __shared__ unsigned long long s_a[DEV_ACC_BINS];
    if (threadIdx.x < DEV_ACC_BINS) s_a[threadIdx.x] = 0;
    __syncthreads();
    DevTargetAcc a;
    for (int i = blockIdx.x * DEV_T + threadIdx.x; i < n; i += gridDim.x * DEV_T) {
        const int st = status[i];
        a.cnt[0] += st == PPP_DEV_MATCHED; a.cnt[1] += st == PPP_DEV_TOO_FAR; a.cnt[2] += st == PPP_DEV_NO_NORMAL; a.cnt[3] += st == PPP_DEV_DROPPED;
        if (st != PPP_DEV_MATCHED) { deviation[i] = dev_nan(); v[i] = dev_nan(); target[i] = 0.0; continue; }
        const double x = v[i], over = x - allowance;
        target[i] = over > 0.0 ? gain * over : 0.0;
        a.add(x, allowance, d2[i]);
    }
    a.flush(s_a, acc);
}

/* the bin of x in the histogram over [-span, span]: min(63, max(0, floor((x / span + 1) 32))), bin 32 when span == 0 */
__host__ __device__ inline int dev_bin(double x, double span)
{
    if (!(span > 0.0)) return PPP_CONTACT_BINS / 2;
    const double f = floor((x / span + 1.0) * (double)(PPP_CONTACT_BINS / 2));
    return f < 0.0 ? 0 : (f > (double)(PPP_CONTACT_BINS - 1) ? PPP_CONTACT_BINS - 1 : (int)f);
}

/* second phase, behind the first: the histogram over [-span, span], span = max(|min v|, |max v|) from the first phase's keys
   -- dev_bin -- with per-workgroup LDS bins and one
   integer atomic per non-empty bin, and the sums of v v and of the target as k_prem_stats adds them: workgroup g takes the
   contiguous part [g per, (g + 1) per) of the maps, every thread its strided share in index order, block_tree_sum over the
   threads, psq[g] / ptarget[g] for the host to add in order. */
__global__ void __launch_bounds__(PCON_T) k_dev_stats(const unsigned char *__restrict__ status, const double *__restrict__ v,
        const double *__restrict__ target, int n, int per, unsigned long long *acc, double *__restrict__ psq, double *__restrict__ ptarget)
{
    __shared__ int s_bin[PPP_CONTACT_BINS];
    __shared__ double s_sq[PCON_T], s_tg[PCON_T];
    if (threadIdx.x < PPP_CONTACT_BINS) s_bin[threadIdx.x] = 0;
    __syncthreads();
    double span = 0.0;
    if (acc[DEV_ACC_MAX]) span = fmax(fabs(-ordered_unkey64(acc[DEV_ACC_NMIN])), fabs(ordered_unkey64(acc[DEV_ACC_MAX])));
    const int i0 = blockIdx.x * per, i1 = min(n, i0 + per);
    double sq = 0.0, tg = 0.0;
    for (int i = i0 + threadIdx.x; i < i1; i += PCON_T) {
        if (status[i] != PPP_DEV_MATCHED) continue;
        const double x = v[i];
        sq += x * x; tg += target[i];
        atomicAdd(&s_bin[dev_bin(x, span)], 1);
    }
    block_tree_sum(s_sq, sq, s_tg, tg);
    if (threadIdx.x < PPP_CONTACT_BINS && s_bin[threadIdx.x]) atomicAdd(acc + DEV_ACC_BINS + threadIdx.x, (unsigned long long)s_bin[threadIdx.x]);
    if (threadIdx.x == 0) { psq[blockIdx.x] = s_sq[0]; ptarget[blockIdx.x] = s_tg[0]; }
}
