/*
 * ppp_contact.h -- the contact queries on a finished pass or a resident cloud:
 * coverage, path coverage, path contacts and the contact field.  All of them evaluate the contact
 * model of ppp_dynamic.h (Area2Cloud: one wave per evaluation) at many points side by side and
 * reduce what the balls hold; none of them is on a pass's timed path.
 */
#pragma once
#include "ppp_dynamic.h"
#include "../../include/ppp_hip.h" /* PPP_CONTACT_BINS */
/* The kernels of this header are ppp_contact.hip's.  ppp_scan.hip needs the header for its types and device helpers only
   (TileRange, ordered_key, block_tree_sum, ...) and defines PPP_CONTACT_KERNELS_FOREIGN: the kernels are templates there and,
   never launched, never instantiated (PPP_KERNEL's idiom, ppp_kernels.h). */
#ifdef PPP_CONTACT_KERNELS_FOREIGN
#define PPP_CONTACT_KERNEL template <typename PPP_NEVER_ = void> __global__
#else
#define PPP_CONTACT_KERNEL __global__
#endif

/* The knots of the slices' paths (the host fills it: knot_table). */
struct SliceKnots { const float *ky, *kx, *kz; int mm; };
struct KnotTable {
    const float *node_x, *node_y, *node_z;
    const int *node_start, *node_cnt;
    int node_cap;
    __device__ inline SliceKnots at(int st, int mm) const { return SliceKnots{node_y + st, node_x + st, node_z + st, mm}; }
    /* slice s's knots.  K.mm < 3: the slice has no spline, K's pointers are not to be read (B.15).  false: its table lies
       outside the node buffer (refusal bit 2) */
    __device__ inline bool slice(int s, SliceKnots &K) const
    {
        const int st = node_start[s], mm = node_cnt[s];
        K = at(st, mm);
        return mm < 3 || (st >= 0 && (long long)st + mm <= (long long)node_cap);
    }
};

/* compute_boundary's sample at dy on a slice's knots and its ball: the spline point in double, cast to float as Area2Cloud
   casts it, both x-extrema of its contact ellipse, and comput_lan = (for_min->x - boundpoint_it->x) / 2 in float (negative);
   PCL squares it: the float r * r.  A NaN r2 holds no point (FLANN: no distance is <= NaN, B.16).  kk: the neighbours the
   search found, which L.sel still lists. */
struct SampleBall { float qx, qy, qz, r, r2; int kk; };
__device__ inline SampleBall wave_sample_ball(const ContactIndex &I, const SlabView &V, const DynGrid &G, DynWaveLds &L, const float2 *ell,
                                              const DynParams &D, const SliceKnots &K, double dy)
{
    double point[3];
    spline_point_f(K.ky, K.kx, K.kz, K.mm, dy, point);
    StampCtx sc; sc.begin(15, false);
    float b[3], ext[2];
    SampleBall B;
    B.kk = wave_area2cloud<true>(V, G, L, I.normals4, ell, D, point, 0, b, sc, ext);
    B.r = (ext[0] - ext[1]) / 2; B.r2 = B.r * B.r;
    B.qx = (float)point[0]; B.qy = (float)point[1]; B.qz = (float)point[2];
    return B;
}

/* what a slice-range handle indexes: the points with x in [incl_lo, incl_hi] of a cloud that spans [mn_x, mx_x] */
struct PCovRange { float incl_lo, incl_hi, mn_x, mx_x, normal_radius; int check; };

/* With R.check (a slice-range handle) every search a sample makes -- the k-NN of Area2Cloud, the normal neighbourhoods of
   those neighbours and the ball -- must lie inside the indexed interval, unless that reaches the cloud's end (the DERR_MARGIN
   test of the waypoints, ppp_kernels.h).  True, in every lane, where one does not: refusal bit 1 (B.22, B.26). */
__device__ inline bool wave_ball_leaves_range(const SlabView &V, const DynWaveLds &L, const DynParams &D, const PCovRange &R,
                                              const SampleBall &B)
{
    if (!(R.check && B.qx == B.qx && B.qy == B.qy && B.qz == B.qz)) return false;
    const int lane = threadIdx.x & 63;
    /* fewer than k neighbours in the indexed part: the whole cloud may hold more */
    float lo = B.kk < D.k ? -INFINITY : INFINITY, hi = B.kk < D.k ? INFINITY : -INFINITY;
    if (lane < B.kk) {
        const float4 c = V.at(L.sel[lane]);
        const float dq = sqrtf(dist2_flann(B.qx, B.qy, B.qz, c.x, c.y, c.z)) * 1.0001f;
        lo = fminf(lo, fminf(B.qx - dq, c.x - R.normal_radius * 1.0001f));
        hi = fmaxf(hi, fmaxf(B.qx + dq, c.x + R.normal_radius * 1.0001f));
    }
    if (B.r2 == B.r2) { lo = fminf(lo, B.qx - fabsf(B.r) * 1.0001f); hi = fmaxf(hi, B.qx + fabsf(B.r) * 1.0001f); }
    lo = wave_min(lo); hi = wave_max(hi);
    return (lo < R.incl_lo && R.incl_lo > R.mn_x) || (hi > R.incl_hi && R.incl_hi < R.mx_x);
}

/* What a tile evaluates and what it owns: the indexed points with x in [ev_lo, ev_hi] are evaluated,
   those with own_lo <= x < own_hi are the handle's own (the cuts between the slices of its range and their neighbours; the
   evaluated interval is the owned one widened by a halo).  The whole cloud: -INFINITY / INFINITY twice. */
struct TileRange {
    float ev_lo, ev_hi, own_lo, own_hi;
    __host__ __device__ inline bool evaluated(float x) const { return x >= ev_lo && x <= ev_hi; }
    __host__ __device__ inline bool owned(float x) const { return x >= own_lo && x < own_hi; }
};

/* a float as an unsigned that orders like it (NaN aside); 0 is below every key of a number and stands for "none" */
__host__ __device__ inline unsigned ordered_key(float f) { unsigned u; __builtin_memcpy(&u, &f, 4); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__host__ __device__ inline float ordered_unkey(unsigned k) { k = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k; float f; __builtin_memcpy(&f, &k, 4); return f; }

/* the largest of a wave's unsigned words, in every lane: ordered keys, counts, the bit patterns of doubles >= +0 (which order as
   their bits do) and, for a minimum, their complements */
template <typename U>
__device__ inline U wave_max_bits(U v)
{
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return v;
}

/* The fixed-order sum of a map's part over a workgroup of PCON_T threads (B.30, B.46): every thread hands in the sum of its
   strided share, added in index order; the tree below adds the threads in one fixed order and leaves the result in s[0] (s:
   PCON_T doubles of LDS).  The same tree gives the same bits; the host adds the workgroups' parts in order.  The four-argument
   form sums a second value (s2, v2) in the same tree steps, on the same barriers; which form is compiled is fixed by the
   overload, so the loop has no test on it.  A barrier ahead of the first read and one behind the last: the LDS writes before
   the call are visible after it. */
#define PCON_T 256
template <bool TWO>
__device__ inline void block_tree_sums(double *s, double v, double *s2, double v2)
{
    s[threadIdx.x] = v;
    if (TWO) s2[threadIdx.x] = v2;
    __syncthreads();
    for (int o = PCON_T / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) { s[threadIdx.x] += s[threadIdx.x + o]; if (TWO) s2[threadIdx.x] += s2[threadIdx.x + o]; }
        __syncthreads();
    }
}
__device__ inline void block_tree_sum(double *s, double v) { block_tree_sums<false>(s, v, nullptr, 0.0); }
__device__ inline void block_tree_sum(double *s, double v, double *s2, double v2) { block_tree_sums<true>(s, v, s2, v2); }

/* ------------------------------------------------------------------ */
/* Coverage (path_generater::compute_coverage / get_coverage, Path_Generation.cpp:463-496, 757-771).  Every            */
/* Area2Cloud(point, 1, 0) of compute_boundary marks the cloud points within half the x-extent of the point's contact   */
/* ellipse.  In Contact_Path_Generation (:711-725) that is every slice's raw path (:719) and the adjusted path of slice */
/* s-1 in dynamic_adjust_path of slice s (:590): raw(0..S-1) and adjusted(1..S-2), all known once the pass is done, so */
/* one launch evaluates all of those balls side by side and marks their points, and a second counts the flags.         */
/* ------------------------------------------------------------------ */

/* The slabs and the y-buckets a ball of radius r about (qx, qy) can touch, padded against the rounding of the float
   positions; every search of the unit over a ball's points (wave_ball_candidates, k_reg_link) begins here.  window: slab bb's
   positions in those buckets, [a, e), a superset of the slab's points with y in the padded interval -- the caller tests the
   distance.  s0 = slab_start[bb].  The y-bucket table is always there: make_plan allocates slab_ytab for every plan (B >= 1)
   and no query gets as far as a launch without a plan, so there is no bisection of the slab's rows here as wave_knn has one. */
struct BallSlabs {
    int blo, bhi, q0, q1;
    __device__ inline void window(const int *__restrict__ ytab, int bb, int s0, int &a, int &e) const
    {
        const int *T = ytab + (size_t)bb * (YTB + 1);
        a = s0 + T[q0]; e = s0 + T[q1];
    }
};
__device__ inline BallSlabs ball_slabs(const DynGrid &G, float qx, float qy, float r)
{
    const float pady = 1e-5f * (fabsf(qy) + r) + 1e-6f, padx = 1e-5f * (fabsf(qx) + r) + 1e-6f;
    return BallSlabs{dyn_slab_of(G, qx - r - padx), dyn_slab_of(G, qx + r + padx), dyn_ybucket(G, qy - r - pady),
                     dyn_ybucket(G, qy + r + pady) + 1};
}

/* The ball walk, all 64 lanes together: visit(c) for every indexed point c in the y-windows of the slabs the ball touches
   (ball_slabs), as in wave_knn -- 64 slabs a round, a lane per slab finds its window, an exclusive prefix of the windows' sizes
   goes to L.off and their first positions to L.w0 (all that is used of L: DynWaveLds or the small DwellWaveLds), then the lanes
   stride over the flat positions and bisect L.off for the window of each.  A window lists a point once and the slabs' windows
   are disjoint, so a point is visited once; which lane visits it is fixed, the order among lanes is not: visit may set flags
   or add integers, nothing whose result depends on an order.  Wave barriers only. */
template <typename Lds, typename Visit>
__device__ __attribute__((always_inline)) inline void wave_ball_candidates(const SlabView &V, const DynGrid &G, Lds &L, float qx, float qy,
                                                                          float r, Visit &&visit)
{
    const int lane = threadIdx.x & 63;
    const BallSlabs S = ball_slabs(G, qx, qy, r);
    for (int cb = S.blo; cb <= S.bhi; cb += 64) {
        const int bb = cb + lane;
        int a = 0, e = 0;
        if (bb <= S.bhi) S.window(V.ytab, bb, V.slab_start[bb], a, e);
        const int cnt = e - a;
        int inc = cnt;
        for (int o = 1; o < 64; o <<= 1) { const int v = __shfl_up(inc, o, 64); if (lane >= o) inc += v; }
        const int T = __shfl(inc, 63, 64);
        __builtin_amdgcn_wave_barrier(); /* the round before has read its windows */
        L.off[lane] = inc - cnt; L.w0[lane] = a;
        __builtin_amdgcn_wave_barrier();
        __threadfence_block();
        const int wtop = S.bhi - cb < 63 ? S.bhi - cb : 63;
        for (int t = lane; t < T; t += 64) {
            int lo = 0, hi = wtop; /* the window holding flat position t */
            while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (L.off[mid] <= t) lo = mid; else hi = mid - 1; }
            visit(V.at(L.w0[lo] + (t - L.off[lo])));
        }
    }
}

/* kdtree.radiusSearch(centre, r): flags[i] = 1 for every indexed point within the ball (dist2_flann <= r2, the float
   square of r as PCL hands it to FLANN), by the ball walk.  Points are only ever set to 1, so balls that overlap need no
   atomics. */
__device__ inline void wave_mark_ball(const SlabView &V, const DynGrid &G, DynWaveLds &L, float qx, float qy, float qz, float r,
                                      float r2, unsigned char *__restrict__ flags)
{
    wave_ball_candidates(V, G, L, qx, qy, r, [&](const float4 &c) {
        if (dist2_flann(qx, qy, qz, c.x, c.y, c.z) <= r2) flags[idx_of(c)] = 1;
    });
}

/* One wave per compute_boundary sample: blockIdx.y = slice, blockIdx.z = 0 the raw path (knots at raw_sc, as k_dyn_first_eval
   found them), 1 the adjusted one (node_start / node_cnt after the pass; slices 1 .. S-2).  The reference's "last point" call
   repeats the last sample's ball; a loop that ran zero times adds no ball. */
PPP_CONTACT_KERNEL void __launch_bounds__(64 * DYN_WAVES) k_cov_balls(ContactIndex I, DynParams D, KnotTable T, const int *__restrict__ raw_sc,
        int maxNB, unsigned char *__restrict__ flags)
{
    __shared__ DynWaveLds s_w[DYN_WAVES];
    __shared__ float2 s_ell[DYN_ELL];
    dyn_stage_ellipse(I.ell_cs, s_ell);
    const DynGrid G = dyn_grid(I.m);
    const int S = I.m->S, err = I.m->err;
    __syncthreads();
    if (err) return;
    const int wv = threadIdx.x >> 6;
    const int s = blockIdx.y, j = blockIdx.x * DYN_WAVES + wv;
    const bool adjusted = blockIdx.z == 1;
    if (s >= S || j >= maxNB || (adjusted && (s < 1 || s > S - 2))) return;
    const SliceKnots K = adjusted ? T.at(T.node_start[s], T.node_cnt[s]) : T.at(raw_sc[2 * s], raw_sc[2 * s + 1]);
    if (K.mm < 3) return;
    const double miny = (double)K.ky[0], maxy = (double)K.ky[K.mm - 1];
    const double dy = dyn_boundary_dy(D, miny, j);
    if (!(dy < maxy - 2)) return;
    const SlabView V = I.view();
    const SampleBall B = wave_sample_ball(I, V, G, s_w[wv], s_ell, D, K, dy);
    if (!(B.r2 == B.r2)) return; /* a NaN radius marks nothing */
    wave_mark_ball(V, G, s_w[wv], B.qx, B.qy, B.qz, fabsf(B.r), B.r2, flags);
}

/* get_coverage's yes count: the flags (0 / 1, zero padding up to a multiple of 16 bytes) summed 16 at a time by population
   count, a wave sum, one atomic per workgroup -- integers, so the count is the same in every run */
#define COV_T 256
PPP_CONTACT_KERNEL void __launch_bounds__(COV_T) k_cov_count(const uint4 *__restrict__ flags16, int n16, int *__restrict__ count)
{
    __shared__ int s_c;
    if (threadIdx.x == 0) s_c = 0;
    __syncthreads();
    int c = 0;
    for (int i = blockIdx.x * COV_T + threadIdx.x; i < n16; i += gridDim.x * COV_T) {
        const uint4 w = flags16[i];
        c += __popc(w.x) + __popc(w.y) + __popc(w.z) + __popc(w.w);
    }
    c = wave_sum(c);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(&s_c, c);
    __syncthreads();
    if (threadIdx.x == 0 && s_c) atomicAdd(count, s_c);
}

/* ------------------------------------------------------------------ */
/* Path coverage (ppp_get_path_coverage): the same contact model applied to the paths a pass ends with --    */
/* every slice's final knots (node_start / node_cnt after the pass: adjusted where the adjustment ran), for every walk.     */
/* One launch marks the balls (k_pcov_balls), k_cov_count counts the flags.                                                */
/* ------------------------------------------------------------------ */

/* Slice sb + blockIdx.y, one wave per compute_boundary sample: wave w takes samples j = blockIdx.x * DYN_WAVES + w,
   j + gridDim.x * DYN_WAVES, ... while dy < maxy - 2 (a loop that runs zero times adds no ball, B.15).  The ball of a sample
   is k_cov_balls's.  err[0] |= 1 where a sample's searches leave a slice-range handle's interval (wave_ball_leaves_range),
   err[0] |= 2 for a knot table beyond node_cap.  The host then refuses the answer. */
PPP_CONTACT_KERNEL void __launch_bounds__(64 * DYN_WAVES) k_pcov_balls(ContactIndex I, DynParams D, KnotTable T, int sb, PCovRange R,
        unsigned char *__restrict__ flags, int *__restrict__ err)
{
    __shared__ DynWaveLds s_w[DYN_WAVES];
    __shared__ float2 s_ell[DYN_ELL];
    dyn_stage_ellipse(I.ell_cs, s_ell);
    const DynGrid G = dyn_grid(I.m);
    SliceKnots K;
    const bool in_table = T.slice(sb + blockIdx.y, K);
    __syncthreads();
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (K.mm < 3) return;
    if (!in_table) { if (threadIdx.x == 0 && blockIdx.x == 0) atomicOr(err, 2); return; }
    const double miny = (double)K.ky[0], maxy = (double)K.ky[K.mm - 1];
    const SlabView V = I.view();
    DynWaveLds &L = s_w[wv];
    for (int j = blockIdx.x * DYN_WAVES + wv; j < (1 << 24); j += gridDim.x * DYN_WAVES) {
        const double dy = dyn_boundary_dy(D, miny, j);
        if (!(dy < maxy - 2)) return;
        const SampleBall B = wave_sample_ball(I, V, G, L, s_ell, D, K, dy);
        if (wave_ball_leaves_range(V, L, D, R, B) && lane == 0) atomicOr(err, 1);
        if (!(B.r2 == B.r2)) continue; /* a NaN radius marks nothing (B.16) */
        wave_mark_ball(V, G, L, B.qx, B.qy, B.qz, fabsf(B.r), B.r2, flags);
    }
    if (lane == 0) atomicOr(err, 2); /* 2^24 samples on one slice: no knot table of a cloud is that long */
}

/* ------------------------------------------------------------------ */
/* Path contacts (ppp_get_path_contacts): how many of k_pcov_balls's balls hold each cloud point, and the   */
/* first and last slice that has one of them.  Point-centric, no atomics on the maps: k_pcon_offsets counts each slice's  */
/* samples, k_pcon_samples evaluates every sample's ball once into a per-slice table, k_pcon_points walks the slab index   */
/* and tests every point against the balls of the slices that reach it, k_pcon_stats reduces the count map.               */
/* ------------------------------------------------------------------ */

/* compute_boundary's sample count on knots from miny to maxy: the first j with !(dyn_boundary_dy(j) < maxy - 2).  dy does not
   decrease with j (tool_radius > 0: the closed form is exact where it is used, the running sum rounds monotonically), so a
   doubling search and a bisection find it on the very values k_pcov_balls's loop tests.  1 << 24 = k_pcov_balls's cap. */
__device__ inline int pcon_sample_count(const DynParams &D, double miny, double maxy)
{
    auto in = [&](int j) { return dyn_boundary_dy(D, miny, j) < maxy - 2; };
    if (!in(0)) return 0;
    int lo = 0, hi = 1; /* in(lo); hi == 1 << 24 or !in(hi) */
    while (hi < (1 << 24) && in(hi)) { lo = hi; hi = hi < (1 << 23) ? 2 * hi : (1 << 24); }
    while (hi - lo > 1) { const int mid = lo + (hi - lo) / 2; if (in(mid)) lo = mid; else hi = mid; }
    return hi;
}

/* One workgroup: off[i] = the first table row of slice sb + i, off[nsl] = the rows in all, off[nsl + 1] = the refusal word
   after this launch.  A slice of fewer than 3 knots has none (B.15).  err |= 2 for a knot table beyond node_cap or a slice
   of 2^24 samples (k_pcov_balls's refusals), 4 for a slice of 2^22 samples or a table of 2^30 rows or more. */
PPP_CONTACT_KERNEL void __launch_bounds__(PCON_T) k_pcon_offsets(DynParams D, KnotTable T, int sb, int nsl, int *__restrict__ off,
        int *__restrict__ err)
{
    __shared__ int s_scan[17];
    long long run = 0;
    for (int base = 0; base < nsl; base += PCON_T) {
        const int i = base + threadIdx.x;
        int c = 0;
        if (i < nsl) {
            SliceKnots K;
            const bool in_table = T.slice(sb + i, K);
            if (K.mm >= 3) {
                if (!in_table) atomicOr(err, 2);
                else {
                    c = pcon_sample_count(D, (double)K.ky[0], (double)K.ky[K.mm - 1]);
                    if (c >= (1 << 24)) { atomicOr(err, 2); c = 0; }
                    else if (c >= (1 << 22)) { atomicOr(err, 4); c = 0; }
                }
            }
        }
        int tot;
        const int pre = block_exscan(c, s_scan, &tot);
        if (run + tot >= (1ll << 30)) { if (threadIdx.x == 0) atomicOr(err, 4); tot = 0; }
        else if (i < nsl) off[i] = (int)run + pre;
        run += tot;
    }
    __syncthreads();
    if (threadIdx.x == 0) { off[nsl] = (int)run; off[nsl + 1] = atomicOr(err, 0); }
}

/* Slice sb + s0 + blockIdx.y, one wave per sample (j = blockIdx.x * DYN_WAVES + wave, strided): the ball of k_pcov_balls
   (same spline point, same Area2Cloud, r = (ext[0] - ext[1]) / 2 and r * r in float) goes to tab[off + j] as (qx, qy, qz,
   r2); a NaN r2 holds no point.  reach[3 i ..] takes the slice's x-reach and largest |r| as keys (ordered_key; the lower end
   as the key of its negation), one atomic per workgroup each.  The refusal of k_pcov_balls (wave_ball_leaves_range). */
PPP_CONTACT_KERNEL void __launch_bounds__(64 * DYN_WAVES) k_pcon_samples(ContactIndex I, DynParams D, KnotTable T, const int *__restrict__ off,
        int sb, int s0, PCovRange R, float4 *__restrict__ tab, unsigned *__restrict__ reach, int *__restrict__ err)
{
    __shared__ DynWaveLds s_w[DYN_WAVES];
    __shared__ float2 s_ell[DYN_ELL];
    __shared__ unsigned s_reach[3];
    dyn_stage_ellipse(I.ell_cs, s_ell);
    const DynGrid G = dyn_grid(I.m);
    const int i = s0 + blockIdx.y, s = sb + i;
    const int o0 = off[i], cnt = off[i + 1] - o0;
    if (threadIdx.x < 3) s_reach[threadIdx.x] = 0;
    __syncthreads();
    if (cnt <= 0) return; /* the whole workgroup: no knots, too few, or refused by k_pcon_offsets */
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const SliceKnots K = T.at(T.node_start[s], T.node_cnt[s]); /* (inside the table: k_pcon_offsets counted its samples) */
    const double miny = (double)K.ky[0];
    const SlabView V = I.view();
    DynWaveLds &L = s_w[wv];
    float nlo = -INFINITY, hi = -INFINITY, rmax = -INFINITY; /* the wave's: -min(qx - |r|), max(qx + |r|), max |r| */
    for (int j = blockIdx.x * DYN_WAVES + wv; j < cnt; j += gridDim.x * DYN_WAVES) {
        const SampleBall B = wave_sample_ball(I, V, G, L, s_ell, D, K, dyn_boundary_dy(D, miny, j));
        if (wave_ball_leaves_range(V, L, D, R, B) && lane == 0) atomicOr(err, 1);
        if (lane == 0) tab[o0 + j] = make_float4(B.qx, B.qy, B.qz, B.r2);
        if (B.r2 == B.r2 && B.qx == B.qx && B.qz == B.qz) { /* a ball that can hold a point */
            nlo = fmaxf(nlo, fabsf(B.r) - B.qx); hi = fmaxf(hi, B.qx + fabsf(B.r)); rmax = fmaxf(rmax, fabsf(B.r));
        }
    }
    if (lane == 0 && rmax >= 0.f) { atomicMax(&s_reach[0], ordered_key(nlo)); atomicMax(&s_reach[1], ordered_key(hi)); atomicMax(&s_reach[2], ordered_key(rmax)); }
    __syncthreads();
    if (threadIdx.x < 3 && s_reach[threadIdx.x]) atomicMax(reach + 3 * i + threadIdx.x, s_reach[threadIdx.x]);
}

/* The point walk.  One thread per position of the slab index, PCON_T consecutive positions a round (one x-interval, a slab or
   two): the slices whose reach, padded as ball_slabs pads, meets the round's x-interval are listed in LDS; for each, the point
   bisects the slice's table for qy >= y - rmax - pad (qy does not decrease with j) and walks to qy > y + rmax + pad;
   held(acc, k, j, d2, r2) for every row j, of listed slice k, whose ball holds the point (d2 = dist2_flann(q, p) <= r2), then
   store(acc, p) once per point.  acc is the caller's Acc, made anew for every point and kept in registers; store writes it at
   the point's cloud index (idx_of) if a ball held the point -- the caller's own test, on what it gathered, so that the walk
   keeps no flag of its own beside the caller's count.  block_exscan lists the slices in ASCENDING order and a slice's rows are
   walked upwards, so a point meets its balls in ascending (slice, sample) order: a float sum that held adds in that order is
   the same in every run (B.45) -- keep the listing ordered.  All threads of the workgroup call (two barriers a round). */
template <typename Acc, typename Held, typename Store>
__device__ __attribute__((always_inline)) inline void pcon_walk_points(const DevMeta *m, const float4 *__restrict__ sorted4,
        const float4 *__restrict__ tab, const int *__restrict__ off, const unsigned *__restrict__ reach, int nsl, Held &&held, Store &&store)
{
    __shared__ int s_scan[17];
    __shared__ float s_x[2][PCON_T / 64];
    __shared__ int s_k[PCON_T];
    __shared__ float4 s_sl[PCON_T]; /* lo, hi, rmax of listed slice e; w: its first table row (bits) */
    const int total = m->n_sorted;
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int c0 = blockIdx.x * PCON_T; c0 < total; c0 += gridDim.x * PCON_T) {
        const int pi = c0 + threadIdx.x;
        const bool have = pi < total;
        const float4 p = have ? sorted4[pi] : make_float4(0.f, 0.f, 0.f, 0.f);
        const float wmn = wave_min(have ? p.x : INFINITY), wmx = wave_max(have ? p.x : -INFINITY);
        __syncthreads(); /* the round before has read its lists */
        if (lane == 0) { s_x[0][wv] = wmn; s_x[1][wv] = wmx; }
        __syncthreads();
        float cmn = s_x[0][0], cmx = s_x[1][0];
        for (int w = 1; w < PCON_T / 64; ++w) { cmn = fminf(cmn, s_x[0][w]); cmx = fmaxf(cmx, s_x[1][w]); }
        const float cabs = fmaxf(fabsf(cmn), fabsf(cmx));
        Acc acc;
        const float padp = 1e-5f * fabsf(p.x) + 1e-6f, padq = 1e-5f * fabsf(p.y) + 1e-6f;
        for (int b0 = 0; b0 < nsl; b0 += PCON_T) {
            const int k = b0 + threadIdx.x;
            int take = 0;
            float lo = 0.f, hi = 0.f, rm = 0.f;
            if (k < nsl) {
                const unsigned kh = reach[3 * k + 1];
                if (kh) {
                    lo = -ordered_unkey(reach[3 * k]); hi = ordered_unkey(kh); rm = ordered_unkey(reach[3 * k + 2]);
                    const float pad = 1e-5f * (cabs + rm) + 1e-6f;
                    take = (lo - pad <= cmx && hi + pad >= cmn) ? 1 : 0;
                }
            }
            int nt;
            const int at = block_exscan(take, s_scan, &nt);
            if (take) { s_k[at] = k; s_sl[at] = make_float4(lo, hi, rm, __int_as_float(off[k])); }
            __syncthreads();
            if (!have) continue;
            for (int e = 0; e < nt; ++e) {
                const float4 sl = s_sl[e];
                const int k2 = s_k[e];
                const float rm2 = sl.z;
                const float padx = padp + 1e-5f * rm2;
                if (p.x < sl.x - padx || p.x > sl.y + padx) continue;
                const float ry = rm2 + padq + 1e-5f * rm2;
                const float ylo = p.y - ry, yhi = p.y + ry;
                int a = __float_as_int(sl.w), z = off[k2 + 1];
                const int end = z;
                while (a < z) { const int mid = (a + z) >> 1; if (tab[mid].y < ylo) a = mid + 1; else z = mid; }
                for (int j = a; j < end; ++j) {
                    const float4 t = tab[j];
                    if (t.y > yhi) break;
                    const float d2 = dist2_flann(t.x, t.y, t.z, p.x, p.y, p.z);
                    if (d2 <= t.w) held(acc, k2, j, d2, t.w);
                }
            }
        }
        if (have) store(acc, p);
    }
}

/* The count map by the point walk (pcon_walk_points): how many balls hold the point, and the first and last slice that has
   one of them.  Points that no ball holds keep the 0 / -1 of the memset. */
struct PconAcc { unsigned cnt = 0; int fs = -1, ls = -1; };
PPP_CONTACT_KERNEL void __launch_bounds__(PCON_T) k_pcon_points(const DevMeta *m, const float4 *__restrict__ sorted4, const float4 *__restrict__ tab,
        const int *__restrict__ off, const unsigned *__restrict__ reach, int sb, int nsl, unsigned *__restrict__ counts,
        int *__restrict__ first, int *__restrict__ last)
{
    pcon_walk_points<PconAcc>(m, sorted4, tab, off, reach, nsl,
        [&](PconAcc &a, int k, int, float, float) { ++a.cnt; const int sg = sb + k; a.fs = a.fs < 0 ? sg : min(a.fs, sg); a.ls = max(a.ls, sg); },
        [&](const PconAcc &a, const float4 &p) { if (a.cnt) { const int id = idx_of(p); counts[id] = a.cnt; first[id] = a.fs; last[id] = a.ls; } });
}

/* The statistics of the count map: bins 1 .. 63 of the histogram (bin 0 is n - covered), covered, multi_slice (last >
   first), the sum and the largest count.  Per-workgroup LDS bins, then one integer atomic per non-empty bin and workgroup, as
   k_cov_count counts: the same result in every run.  acc[0 .. 63] bins, [64] covered, [65] multi_slice, [66] total,
   [67] max; workgroup 0 also copies the refusal word into [68], so that one read brings everything back. */
PPP_CONTACT_KERNEL void __launch_bounds__(PCON_T) k_pcon_stats(const unsigned *__restrict__ counts, const int *__restrict__ first,
        const int *__restrict__ last, int n, const int *__restrict__ err, unsigned long long *__restrict__ acc)
{
    __shared__ int s_bin[PPP_CONTACT_BINS];
    __shared__ int s_cov, s_multi;
    __shared__ unsigned s_max;
    __shared__ unsigned long long s_tot;
    if (threadIdx.x < PPP_CONTACT_BINS) s_bin[threadIdx.x] = 0;
    if (threadIdx.x == 0) { s_cov = 0; s_multi = 0; s_max = 0; s_tot = 0; }
    __syncthreads();
    int cov = 0, multi = 0;
    unsigned mx = 0;
    unsigned long long tot = 0;
    const int lane = threadIdx.x & 63;
    for (int b0 = blockIdx.x * PCON_T; b0 < n; b0 += gridDim.x * PCON_T) { /* b0 is the workgroup's: whole waves vote below */
        const int i = b0 + threadIdx.x;
        const unsigned c = i < n ? counts[i] : 0u;
        const int bin = c ? (int)min(c, (unsigned)PPP_CONTACT_BINS - 1) : -1;
        if (c) { ++cov; tot += c; mx = max(mx, c); multi += last[i] > first[i] ? 1 : 0; }
        /* a wave's counts take few values: one LDS add per value present, not per point */
        u64 todo = __ballot(bin >= 0);
        while (todo) {
            const int lead = __ffsll((long long)todo) - 1;
            const int v = __shfl(bin, lead, 64);
            const u64 same = __ballot(bin == v);
            if (lane == lead) atomicAdd(&s_bin[v], __popcll(same));
            todo &= ~same;
        }
    }
    cov = wave_sum(cov); multi = wave_sum(multi); tot = wave_sum(tot);
    mx = wave_max_bits(mx);
    if ((threadIdx.x & 63) == 0) {
        if (cov) { atomicAdd(&s_cov, cov); atomicAdd(&s_tot, tot); atomicMax(&s_max, mx); }
        if (multi) atomicAdd(&s_multi, multi);
    }
    __syncthreads();
    if (threadIdx.x > 0 && threadIdx.x < PPP_CONTACT_BINS && s_bin[threadIdx.x]) atomicAdd(acc + threadIdx.x, (unsigned long long)s_bin[threadIdx.x]);
    if (threadIdx.x == 0 && s_cov) { atomicAdd(acc + 64, (unsigned long long)s_cov); atomicAdd(acc + 66, s_tot); atomicMax(acc + 67, (unsigned long long)s_max); }
    if (threadIdx.x == 0 && s_multi) atomicAdd(acc + 65, (unsigned long long)s_multi);
    if (threadIdx.x == 0 && blockIdx.x == 0) acc[68] = (unsigned long long)(unsigned)*err;
}

/* ------------------------------------------------------------------ */
/* Contact field (ppp_get_contact_field): compute_transform + Area2Cloud AT every cloud point -- principal   */
/* curvatures and the half width r of the contact ellipse.  k_field_batch: a wave per 16 consecutive positions of the slab   */
/* index, one search per point for both extrema, the wave-uniform eigen solve and axes once per batch with a lane per point.  */
/* k_field_waves, one wave per query, is ppp_principal_curvatures_at.  A workgroup that stages a run's candidates in LDS     */
/* and selects from there was built and measured slower.                                                      */
/* ------------------------------------------------------------------ */

/* ppp_principal_curvatures_at: one wave per query q_xyz[3 j ..], wave_area2cloud<true, true> as k_pcon_samples calls it; row j
   of curv5 (and of half_width, where one is given) is query j's. */
PPP_CONTACT_KERNEL void __launch_bounds__(64 * DYN_WAVES) k_field_waves(ContactIndex I, DynParams D, const float *__restrict__ q_xyz, int k,
        float *__restrict__ curv5, float *__restrict__ half_width)
{
    __shared__ DynWaveLds s_w[DYN_WAVES];
    __shared__ float2 s_ell[DYN_ELL];
    dyn_stage_ellipse(I.ell_cs, s_ell);
    __syncthreads();
    const int wv = threadIdx.x >> 6;
    const int j = blockIdx.x * DYN_WAVES + wv;
    if (j >= k) return;
    const SlabView V = I.view();
    const DynGrid G = dyn_grid(I.m);
    const double p[3] = {(double)q_xyz[3 * j], (double)q_xyz[3 * j + 1], (double)q_xyz[3 * j + 2]};
    const size_t row = (size_t)j;
    float bnd[3], ext[2], c5[5];
    StampCtx sc; sc.begin(15, false);
    wave_area2cloud<true, true>(V, G, s_w[wv], I.normals4, s_ell, D, p, 0, bnd, sc, ext, c5);
    if ((threadIdx.x & 63) == 0) {
        if (curv5) { float *o = curv5 + 5 * row; o[0] = c5[0]; o[1] = c5[1]; o[2] = c5[2]; o[3] = c5[3]; o[4] = c5[4]; }
        if (half_width) half_width[row] = (ext[0] - ext[1]) / 2;
    }
}

/* The field proper: a wave takes FIELD_Q consecutive positions of the slab index.  Each query's search and rank-order sums by the
   whole wave, one after the other (wave_knn, wave_contact_tail part 1), the result parked in the lane of the query's number;
   then the eigen solve and the ellipse axes -- a third of an evaluation's instructions, and the same in all 64 lanes when a wave
   serves one query -- ONCE for the batch, a lane per query (part 2); then each query's two folds by the whole wave (part 3).
   Rows by cloud index, as k_field_waves writes them, and the same bits. */
#define FIELD_Q 16
PPP_CONTACT_KERNEL void __launch_bounds__(64 * DYN_WAVES) k_field_batch(ContactIndex I, DynParams D, int n, float *__restrict__ curv5,
        float *__restrict__ half_width)
{
    __shared__ DynWaveLds s_w[DYN_WAVES];
    __shared__ float2 s_ell[DYN_ELL];
    dyn_stage_ellipse(I.ell_cs, s_ell);
    __syncthreads();
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int base = (blockIdx.x * DYN_WAVES + wv) * FIELD_Q;
    if (base >= n) return;
    const int nq = min(FIELD_Q, n - base);
    const SlabView V = I.view();
    const DynGrid G = dyn_grid(I.m);
    DynWaveLds &L = s_w[wv];
    auto lane_f = [](float v, int r) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), r)); }; /* r is wave-uniform */
    auto lane_d = [](double d, int r) {
        const int lo = __builtin_amdgcn_readlane(__double2loint(d), r), hi = __builtin_amdgcn_readlane(__double2hiint(d), r);
        return __hiloint2double(hi, lo);
    };
    float4 myq = make_float4(0.f, 0.f, 0.f, 0.f);
    if (lane < nq) myq = I.sorted4[base + lane];
    ContactFrame mine = {};
    int mykk = 0;
    StampCtx sc; sc.begin(15, false);
    float bnd[3], ext[2], c5[5];
    for (int qi = 0; qi < nq; ++qi) {
        const float sp[3] = {lane_f(myq.x, qi), lane_f(myq.y, qi), lane_f(myq.z, qi)};
        float nn[3] = {0.f, 0.f, 0.f};
        const int kk = wave_knn(V, G, L, sp[0], sp[1], sp[2], D.k, D.r0, I.normals4, nn, sc);
        ContactFrame F = {};
        if (kk > 0) wave_contact_tail<true, true, 1>(I.m, L, s_ell, D, sp, nn, kk, 0, bnd, sc, ext, c5, &F);
        if (lane == qi) {
            for (int i = 0; i < 6; ++i) mine.cov[i] = F.cov[i];
            for (int i = 0; i < 3; ++i) mine.n0[i] = F.n0[i];
            mykk = kk;
        }
        __builtin_amdgcn_wave_barrier(); /* the next search writes where these sums were read */
    }
    {
        const float sp[3] = {myq.x, myq.y, myq.z}, nn[3] = {0.f, 0.f, 0.f};
        wave_contact_tail<true, true, 2>(I.m, L, s_ell, D, sp, nn, mykk > 0 ? mykk : 1, 0, bnd, sc, ext, c5, &mine);
        if (lane < nq && mykk > 0 && curv5) {
            float *o = curv5 + 5 * (size_t)idx_of(myq);
            o[0] = c5[0]; o[1] = c5[1]; o[2] = c5[2]; o[3] = c5[3]; o[4] = c5[4];
        }
    }
    if (!half_width) return;
    for (int qi = 0; qi < nq; ++qi) {
        if (__builtin_amdgcn_readlane(mykk, qi) <= 0) continue;
        const float sp[3] = {lane_f(myq.x, qi), lane_f(myq.y, qi), lane_f(myq.z, qi)}, nn[3] = {0.f, 0.f, 0.f};
        ContactFrame F = {};
        for (int i = 0; i < 3; ++i) { F.n0[i] = lane_f(mine.n0[i], qi); F.cv[i] = lane_f(mine.cv[i], qi); F.cr[i] = lane_f(mine.cr[i], qi); }
        F.pc0 = lane_f(mine.pc0, qi); F.pc1 = lane_f(mine.pc1, qi);
        F.longAxis = lane_d(mine.longAxis, qi); F.shortAxis = lane_d(mine.shortAxis, qi);
        ext[0] = ext[1] = NAN;
        wave_contact_tail<true, true, 3>(I.m, L, s_ell, D, sp, nn, 1, 0, bnd, sc, ext, c5, &F);
        if (lane == 0) half_width[__builtin_amdgcn_readlane(idx_of(myq), qi)] = (ext[0] - ext[1]) / 2;
    }
}

/* ppp_get_contact_field_tile: k_field_batch over the positions [pos0, n) of the slabs that meet the tile's evaluated interval.
   A lane whose point lies outside that interval takes no part -- no search, neither store -- and every search that is made is
   tested against the indexed interval (wave_ball_leaves_range without a ball: the field marks nothing): err[0] |= 1 where one
   leaves it.  hw_own takes the half widths of the owned points alone (the statistics' map).  A kernel of its own: as one
   template with k_field_batch it cost that kernel two registers (104 -> 106 VGPR). */
PPP_CONTACT_KERNEL void __launch_bounds__(64 * DYN_WAVES) k_field_tile(ContactIndex I, DynParams D, int pos0, int n, TileRange T, PCovRange R,
        float *__restrict__ curv5, float *__restrict__ half_width, float *__restrict__ hw_own, int *__restrict__ err)
{
    __shared__ DynWaveLds s_w[DYN_WAVES];
    __shared__ float2 s_ell[DYN_ELL];
    dyn_stage_ellipse(I.ell_cs, s_ell);
    __syncthreads();
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int base = pos0 + (blockIdx.x * DYN_WAVES + wv) * FIELD_Q;
    if (base >= n) return;
    const int nq = min(FIELD_Q, n - base);
    const SlabView V = I.view();
    const DynGrid G = dyn_grid(I.m);
    DynWaveLds &L = s_w[wv];
    auto lane_f = [](float v, int r) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), r)); }; /* r is wave-uniform */
    auto lane_d = [](double d, int r) {
        const int lo = __builtin_amdgcn_readlane(__double2loint(d), r), hi = __builtin_amdgcn_readlane(__double2hiint(d), r);
        return __hiloint2double(hi, lo);
    };
    float4 myq = make_float4(0.f, 0.f, 0.f, 0.f);
    if (lane < nq) myq = I.sorted4[base + lane];
    const bool ev = lane < nq && T.evaluated(myq.x);
    const u64 evm = __ballot(ev), ownm = __ballot(ev && T.owned(myq.x)); /* the wave's evaluated / owned lanes */
    if (!evm) return;
    ContactFrame mine = {};
    int mykk = 0;
    StampCtx sc; sc.begin(15, false);
    float bnd[3], ext[2], c5[5];
    for (int qi = 0; qi < nq; ++qi) {
        if (!((evm >> qi) & 1)) continue;
        const float sp[3] = {lane_f(myq.x, qi), lane_f(myq.y, qi), lane_f(myq.z, qi)};
        float nn[3] = {0.f, 0.f, 0.f};
        const int kk = wave_knn(V, G, L, sp[0], sp[1], sp[2], D.k, D.r0, I.normals4, nn, sc);
        const SampleBall B = {sp[0], sp[1], sp[2], NAN, NAN, kk};
        if (wave_ball_leaves_range(V, L, D, R, B) && lane == 0) atomicOr(err, 1);
        ContactFrame F = {};
        if (kk > 0) wave_contact_tail<true, true, 1>(I.m, L, s_ell, D, sp, nn, kk, 0, bnd, sc, ext, c5, &F);
        if (lane == qi) {
            for (int i = 0; i < 6; ++i) mine.cov[i] = F.cov[i];
            for (int i = 0; i < 3; ++i) mine.n0[i] = F.n0[i];
            mykk = kk;
        }
        __builtin_amdgcn_wave_barrier(); /* the next search writes where these sums were read */
    }
    {
        const float sp[3] = {myq.x, myq.y, myq.z}, nn[3] = {0.f, 0.f, 0.f};
        wave_contact_tail<true, true, 2>(I.m, L, s_ell, D, sp, nn, mykk > 0 ? mykk : 1, 0, bnd, sc, ext, c5, &mine);
        if (lane < nq && mykk > 0 && curv5) {
            float *o = curv5 + 5 * (size_t)idx_of(myq);
            o[0] = c5[0]; o[1] = c5[1]; o[2] = c5[2]; o[3] = c5[3]; o[4] = c5[4];
        }
    }
    for (int qi = 0; qi < nq; ++qi) {
        if (__builtin_amdgcn_readlane(mykk, qi) <= 0) continue;
        const float sp[3] = {lane_f(myq.x, qi), lane_f(myq.y, qi), lane_f(myq.z, qi)}, nn[3] = {0.f, 0.f, 0.f};
        ContactFrame F = {};
        for (int i = 0; i < 3; ++i) { F.n0[i] = lane_f(mine.n0[i], qi); F.cv[i] = lane_f(mine.cv[i], qi); F.cr[i] = lane_f(mine.cr[i], qi); }
        F.pc0 = lane_f(mine.pc0, qi); F.pc1 = lane_f(mine.pc1, qi);
        F.longAxis = lane_d(mine.longAxis, qi); F.shortAxis = lane_d(mine.shortAxis, qi);
        ext[0] = ext[1] = NAN;
        wave_contact_tail<true, true, 3>(I.m, L, s_ell, D, sp, nn, 1, 0, bnd, sc, ext, c5, &F);
        if (lane == 0) {
            const int id = __builtin_amdgcn_readlane(idx_of(myq), qi);
            half_width[id] = (ext[0] - ext[1]) / 2;
            if ((ownm >> qi) & 1) hw_own[id] = (ext[0] - ext[1]) / 2;
        }
    }
}

/* One thread per position of [pos0, pos1): owned[cloud index] = 1 for a point the tile owns, 2 for an evaluated halo point (0
   of the memset elsewhere); cnt[0] += the owned points, cnt[1] += the evaluated ones (integer atomics, one pair per workgroup). */
PPP_CONTACT_KERNEL void __launch_bounds__(PCON_T) k_tile_mark(const float4 *__restrict__ sorted4, int pos0, int pos1, TileRange T,
        unsigned char *__restrict__ owned, int *__restrict__ cnt)
{
    __shared__ int s_c[2];
    if (threadIdx.x < 2) s_c[threadIdx.x] = 0;
    __syncthreads();
    const int pos = pos0 + blockIdx.x * PCON_T + threadIdx.x;
    int own = 0, ev = 0;
    if (pos < pos1) {
        const float4 p = sorted4[pos];
        ev = T.evaluated(p.x) ? 1 : 0; own = ev && T.owned(p.x) ? 1 : 0;
        if (ev) owned[idx_of(p)] = own ? 1 : 2;
    }
    own = wave_sum(own); ev = wave_sum(ev);
    if ((threadIdx.x & 63) == 0 && ev) { atomicAdd(&s_c[0], own); atomicAdd(&s_c[1], ev); }
    __syncthreads();
    if (threadIdx.x == 0 && s_c[1]) { atomicAdd(cnt, s_c[0]); atomicAdd(cnt + 1, s_c[1]); }
}

/* The statistics of the half-width map.  Workgroup g takes the contiguous part [g per, (g + 1) per) of the map: counts and
   bins with integer atomics (per-workgroup LDS bins, then one atomic per non-empty bin, as k_pcon_stats), the smallest and
   largest |r| as ordered keys, and the part's sum of |r| in double -- every thread its strided share in index order, then
   block_tree_sum -- to psum[g]: the host adds the parts in order, so the sum is the same in every run.
   acc[0 .. 63] bins, [64] valid, [65] narrow (2 |r| < min_width, min_width > 0), [66] key of -min |r|, [67] key of max |r|. */
PPP_CONTACT_KERNEL void __launch_bounds__(PCON_T) k_field_stats(const float *__restrict__ half_width, int n, int per, double tool_radius,
        float min_width, unsigned long long *__restrict__ acc, double *__restrict__ psum)
{
    __shared__ int s_bin[PPP_CONTACT_BINS];
    __shared__ int s_valid, s_narrow;
    __shared__ unsigned s_lo, s_hi;
    __shared__ double s_sum[PCON_T];
    if (threadIdx.x < PPP_CONTACT_BINS) s_bin[threadIdx.x] = 0;
    if (threadIdx.x == 0) { s_valid = 0; s_narrow = 0; s_lo = 0; s_hi = 0; }
    __syncthreads();
    const int i0 = blockIdx.x * per, i1 = min(n, i0 + per);
    int valid = 0, narrow = 0;
    unsigned klo = 0, khi = 0;
    double sum = 0.0;
    for (int i = i0 + threadIdx.x; i < i1; i += PCON_T) {
        const float a = fabsf(half_width[i]);
        if (!(a <= 3.402823466e+38f)) continue; /* NaN or infinite: no width */
        ++valid;
        if (min_width > 0.f && 2.f * a < min_width) ++narrow;
        klo = max(klo, ordered_key(-a)); khi = max(khi, ordered_key(a));
        sum += (double)a;
        int bin = (int)floor((double)a / tool_radius * (double)(PPP_CONTACT_BINS - 1));
        bin = bin < 0 ? 0 : (bin > PPP_CONTACT_BINS - 1 ? PPP_CONTACT_BINS - 1 : bin);
        atomicAdd(&s_bin[bin], 1);
    }
    valid = wave_sum(valid); narrow = wave_sum(narrow);
    klo = wave_max_bits(klo); khi = wave_max_bits(khi);
    if ((threadIdx.x & 63) == 0 && valid) { atomicAdd(&s_valid, valid); atomicAdd(&s_narrow, narrow); atomicMax(&s_lo, klo); atomicMax(&s_hi, khi); }
    block_tree_sum(s_sum, sum);
    if (threadIdx.x < PPP_CONTACT_BINS && s_bin[threadIdx.x]) atomicAdd(acc + threadIdx.x, (unsigned long long)s_bin[threadIdx.x]);
    if (threadIdx.x == 0) {
        psum[blockIdx.x] = s_sum[0];
        if (s_valid) {
            atomicAdd(acc + 64, (unsigned long long)s_valid); atomicAdd(acc + 65, (unsigned long long)s_narrow);
            atomicMax(acc + 66, (unsigned long long)s_lo); atomicMax(acc + 67, (unsigned long long)s_hi);
        }
    }
}
