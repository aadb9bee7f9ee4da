/*
 * ppp_feed.h -- the timed feed schedule (ppp_get_path_feed): for every row of the WayPointsList the
 * dwell factor there (the rows of ppp_get_path_dwell interpolated in y along the slice), the feed the contact point may have
 * under a cap and an acceleration limit, and the time at which the waypoint is reached.  Lengths and times are summed as
 * fixed-point integers (2^-20 mm, 2^-30 s): integer sums have no order.  The envelope is a minimum of exact doubles, which
 * has no order either: every waypoint is independent, and every output is the same bits in every run.  No float atomics, no
 * float sum whose order is not fixed.
 */
#pragma once
#include "ppp_removal.h"

#define FEED_TILE 256                 /* waypoints of a k_feed_env workgroup, and the records of a staged tile: 4 KB of LDS */
#define FEED_LEN_FIXED 1048576.0      /* 2^20: lengths in 2^-20 mm */
#define FEED_TIME_FIXED 1073741824.0  /* 2^30: times in 2^-30 s */

/* what the envelope reads of waypoint j: its arc length on the slice and the square of its cap.  16 bytes, moved as one
   128-bit access from memory and through the LDS */
struct __attribute__((aligned(16))) FeedRec { long long S; double c2; };

/* acc of the call: waypoints by limit 0 .. 3, the largest feed as its bit pattern (a feed is >= +0: such doubles order as
   their bits do), the complement of the smallest one's, then the integer sums: duration, its links, path length, link length */
enum { FEED_ACC_LIMIT = 0, FEED_ACC_MAX = 4, FEED_ACC_NMIN = 5, FEED_ACC_DUR = 6, FEED_ACC_DUR_LINKS = 7, FEED_ACC_PATH = 8, FEED_ACC_LINK = 9,
       FEED_ACC_WORDS = 10 };

/* the double distance of two float points, the differences taken in double; 0 when an end is not finite */
__device__ inline double feed_dist(const float4 a, const float4 b)
{
    if (!(isfinite(a.x) && isfinite(a.y) && isfinite(a.z) && isfinite(b.x) && isfinite(b.y) && isfinite(b.z))) return 0.0;
    const double dx = (double)b.x - (double)a.x, dy = (double)b.y - (double)a.y, dz = (double)b.z - (double)a.z;
    return sqrt(((dx * dx) + dy * dy) + dz * dz);
}

/* exclusive scan of one 64-bit integer per thread across a workgroup of PCON_T threads; *total: the sum.  scratch: PCON_T / 64
   + 1 words of LDS.  Two barriers ahead of the reads, one behind them: the caller may call again at once */
__device__ inline long long feed_block_exscan(long long v, long long *scratch, long long *total)
{
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    long long inc = v;
    for (int o = 1; o < 64; o <<= 1) {
        const long long t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    if (lane == 63) scratch[wid] = inc;
    __syncthreads();
    long long pre = inc - v, tot = 0;
    for (int w = 0; w < PCON_T / 64; ++w) { const long long t = scratch[w]; if (w < wid) pre += t; tot += t; }
    __syncthreads();
    *total = tot;
    return pre;
}

/* One thread per waypoint w of the list (xyz: PPP_STAGE_WP_XYZ's rows).  off[0 .. nk]: the kept slices' first waypoints, so
   slice k holds [off[k], off[k + 1]); a slice without waypoints shares its offset with its successor, and the LAST k with
   off[k] <= w is the one that holds w.  rowoff[0 .. nk]: the kept slices' rows of the dwell table (ry: their float y, rt:
   their factors).  Writes the row's slice, dwell and the limit of the cap (0 dwell, 1 feed_max, 2 end: the lowest number on a
   tie), the cap, the fixed-point length D of the segment to the next waypoint of the slice (0 behind the last), and for a
   slice's last waypoint the link to the next slice that has waypoints: its fixed-point length and time (0 behind the list) */
__global__ void __launch_bounds__(PCON_T) k_feed_map(const float4 *__restrict__ xyz, const int *__restrict__ off, int nk, int W, int first_kept,
        const int *__restrict__ rowoff, const float *__restrict__ ry, const double *__restrict__ rt, double feed, double feed_max, double end_feed,
        double link_feed, ppp_feed_row *__restrict__ rows, double *__restrict__ cap, long long *__restrict__ D, long long *__restrict__ linkD,
        long long *__restrict__ linkT)
{
    const int w = blockIdx.x * PCON_T + threadIdx.x;
    if (w >= W) return;
    int lo = 0, hi = nk - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (off[mid] <= w) lo = mid; else hi = mid - 1; }
    const int k = lo, o = off[k], m = off[k + 1] - o, i = w - o;
    const float4 p = xyz[w];
    const double y = (double)p.y;
    const int r0 = rowoff[k], r1 = rowoff[k + 1];
    double dwell = 1.0;
    if (r1 > r0 && y == y) {
        if (y < (double)ry[r0]) dwell = rt[r0];
        else if (y >= (double)ry[r1 - 1]) dwell = rt[r1 - 1];
        else {
            int a = r0, b = r1 - 2; /* the last row with y_a <= y: row r0 has it, row r1 - 1 has not */
            while (a < b) { const int mid = (a + b + 1) >> 1; if ((double)ry[mid] <= y) a = mid; else b = mid - 1; }
            const double ya = (double)ry[a], yb = (double)ry[a + 1], ta = rt[a], tb = rt[a + 1];
            if (yb == ya) dwell = ta;
            else { const double u = (y - ya) / (yb - ya); dwell = ta + u * (tb - ta); }
        }
    }
    double c = feed / dwell;
    int limit = 0;
    if (feed_max < c) { c = feed_max; limit = 1; }
    if ((i == 0 || i == m - 1) && end_feed >= 0.0 && end_feed < c) { c = end_feed; limit = 2; }
    ppp_feed_row r;
    r.slice = first_kept + k; r.limit = limit; r.dwell = dwell; r.s = 0.0; r.feed = c; r.t = 0.0;
    rows[w] = r;
    cap[w] = c;
    if (i < m - 1) { D[w] = llrint(feed_dist(p, xyz[w + 1]) * FEED_LEN_FIXED); return; }
    D[w] = 0;
    if (w + 1 < W) { /* the next row of the list is the first waypoint of the next slice that has any */
        const double l = feed_dist(p, xyz[w + 1]);
        linkD[k] = llrint(l * FEED_LEN_FIXED);
        linkT[k] = llrint((l / link_feed) * FEED_TIME_FIXED);
    }
}

/* A workgroup per kept slice: S_0 = 0, S_{i + 1} = S_i + D_i in 64-bit integers, PCON_T waypoints a round with a carry; the
   envelope's record (S_i, c_i * c_i) per waypoint and the slice's length */
__global__ void __launch_bounds__(PCON_T) k_feed_scan(const int *__restrict__ off, const long long *__restrict__ D, const double *__restrict__ cap,
        FeedRec *__restrict__ rec, long long *__restrict__ slice_len)
{
    __shared__ long long s_scan[PCON_T / 64 + 1];
    const int k = blockIdx.x, o = off[k], m = off[k + 1] - o;
    long long carry = 0;
    for (int base = 0; base < m; base += PCON_T) {
        const int i = base + (int)threadIdx.x;
        long long tot;
        const long long pre = feed_block_exscan(i < m ? D[o + i] : 0, s_scan, &tot);
        if (i < m) { const double c = cap[o + i]; FeedRec r; r.S = carry + pre; r.c2 = c * c; rec[o + i] = r; }
        carry += tot;
    }
    if (threadIdx.x == 0) slice_len[k] = carry;
}

/* The acceleration envelope, a workgroup per (slice, tile of FEED_TILE waypoints), a thread per waypoint i:
     q_i = min over the slice's j of (c_j^2 + (2 accel) ((double)|S_i - S_j| 2^-20)),  feed_i = sqrt(q_i),  limit 3 where q_i < c_i^2
   Term j = i is c_i^2 itself, c_j^2 >= 0 and a rounding is monotone: a j whose (2 accel) (|S_i - S_j| 2^-20), as rounded, is
   not below c_i^2 cannot lower the minimum.  S is monotone along the slice, so the j that can lie in one stretch around the
   tile: its ends are bisected with that very product against the largest c^2 of the tile (the tile itself always belongs).
   The stretch comes through the LDS a tile of records at a time, one 128-bit store a thread; every thread then reads every
   record, all lanes the same address -- a broadcast, no bank conflict -- and keeps its minimum in registers.  A minimum of
   exact doubles has no order.  accel == +inf: the cap itself.  One row store a thread, no atomics. */
__global__ void __launch_bounds__(FEED_TILE) k_feed_env(const int2 *__restrict__ tiles, const int *__restrict__ off, const FeedRec *__restrict__ rec,
        double accel, ppp_feed_row *__restrict__ rows)
{
    __shared__ FeedRec s_rec[FEED_TILE];
    __shared__ double s_max[FEED_TILE / 64];
    __shared__ int s_j[2];
    const int2 tile = tiles[blockIdx.x];
    const int o = off[tile.x], m = off[tile.x + 1] - o, i0 = tile.y, i1 = min(i0 + FEED_TILE, m) - 1;
    const int i = i0 + (int)threadIdx.x;
    const bool act = i < m;
    FeedRec me; me.S = 0; me.c2 = 0.0;
    if (act) me = rec[o + i];
    double q = me.c2;
    if (accel < INFINITY) {
        double cm = me.c2; /* the tile's largest c^2 (0 from the idle threads: a cap is >= 0) */
        for (int d = 32; d > 0; d >>= 1) cm = fmax(cm, __shfl_xor(cm, d, 64));
        if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = cm;
        __syncthreads();
        const double twoa = 2.0 * accel;
        if (threadIdx.x == 0) {
            cm = s_max[0];
            for (int v = 1; v < FEED_TILE / 64; ++v) cm = fmax(cm, s_max[v]);
            const long long Sa = rec[o + i0].S, Sb = rec[o + i1].S;
            int a = 0, b = i0; /* the first j <= i0 whose product lies below cm: everything from it to i0 does */
            while (a < b) { const int mid = (a + b) >> 1; if (twoa * ((double)(Sa - rec[o + mid].S) * (1.0 / FEED_LEN_FIXED)) < cm) b = mid; else a = mid + 1; }
            s_j[0] = a;
            a = i1; b = m - 1; /* the last j >= i1 whose product lies below cm */
            while (a < b) { const int mid = (a + b + 1) >> 1; if (twoa * ((double)(rec[o + mid].S - Sb) * (1.0 / FEED_LEN_FIXED)) < cm) a = mid; else b = mid - 1; }
            s_j[1] = a;
        }
        __syncthreads();
        const int jlo = s_j[0], jhi = s_j[1];
        for (int jb = jlo; jb <= jhi; jb += FEED_TILE) {
            const int j = jb + (int)threadIdx.x;
            FeedRec r; r.S = 0; r.c2 = INFINITY; /* beyond the stretch: a term that never wins */
            if (j <= jhi) r = rec[o + j];
            s_rec[threadIdx.x] = r;
            __syncthreads();
            if (act) {
#pragma unroll 8
                for (int t = 0; t < FEED_TILE; ++t) {
                    const FeedRec e = s_rec[t];
                    const long long d = me.S - e.S;
                    q = fmin(q, e.c2 + twoa * ((double)(d < 0 ? -d : d) * (1.0 / FEED_LEN_FIXED)));
                }
            }
            __syncthreads();
        }
    }
    if (!act) return;
    ppp_feed_row r = rows[o + i];
    r.s = (double)me.S * (1.0 / FEED_LEN_FIXED);
    if (accel < INFINITY) { r.feed = sqrt(q); if (q < me.c2) r.limit = 3; }
    rows[o + i] = r;
}

/* The times, first phase, a workgroup per kept slice: dt of every segment from the feeds at its ends -- 0 for D == 0,
   2 sqrt((D 2^-20) / accel) from rest to rest, else (2 (D 2^-20)) / (v_i + v_{i + 1}), exact under a constant acceleration --
   as llrint(dt 2^30); the slice's last waypoint carries the link's time.  tloc[w]: the integer sum of the slice's entries
   ahead of w; slice_t[k]: the slice's sum with its link */
__global__ void __launch_bounds__(PCON_T) k_feed_time(const int *__restrict__ off, const ppp_feed_row *__restrict__ rows, const long long *__restrict__ D,
        const long long *__restrict__ linkT, double accel, long long *__restrict__ tloc, long long *__restrict__ slice_t)
{
    __shared__ long long s_scan[PCON_T / 64 + 1];
    const int k = blockIdx.x, o = off[k], m = off[k + 1] - o;
    long long carry = 0;
    for (int base = 0; base < m; base += PCON_T) {
        const int i = base + (int)threadIdx.x;
        long long dtq = 0;
        if (i < m - 1) {
            const long long Dq = D[o + i];
            if (Dq != 0) {
                const double x = (double)Dq * (1.0 / FEED_LEN_FIXED), vs = rows[o + i].feed + rows[o + i + 1].feed;
                const double dt = vs == 0.0 ? 2.0 * sqrt(x / accel) : (2.0 * x) / vs;
                dtq = llrint(dt * FEED_TIME_FIXED);
            }
        } else if (i == m - 1) dtq = linkT[k];
        long long tot;
        const long long pre = feed_block_exscan(dtq, s_scan, &tot);
        if (i < m) tloc[o + i] = carry + pre;
        carry += tot;
    }
    if (threadIdx.x == 0) slice_t[k] = carry;
}

/* second phase, one workgroup: the slices' sums scanned in list order (slice_t becomes each slice's start), and the call's
   integer sums -- the duration, its links, the path length, the link length */
__global__ void __launch_bounds__(PCON_T) k_feed_time_slices(int nk, long long *__restrict__ slice_t, const long long *__restrict__ linkT,
        const long long *__restrict__ slice_len, const long long *__restrict__ linkD, unsigned long long *__restrict__ acc)
{
    __shared__ long long s_scan[PCON_T / 64 + 1];
    long long carry = 0, lt = 0, sl = 0, ld = 0;
    for (int base = 0; base < nk; base += PCON_T) {
        const int k = base + (int)threadIdx.x;
        long long tot;
        const long long pre = feed_block_exscan(k < nk ? slice_t[k] : 0, s_scan, &tot);
        if (k < nk) { slice_t[k] = carry + pre; lt += linkT[k]; sl += slice_len[k]; ld += linkD[k]; }
        carry += tot;
    }
    long long t0, t1, t2;
    feed_block_exscan(lt, s_scan, &t0);
    feed_block_exscan(sl, s_scan, &t1);
    feed_block_exscan(ld, s_scan, &t2);
    if (threadIdx.x == 0) {
        acc[FEED_ACC_DUR] = (unsigned long long)carry; acc[FEED_ACC_DUR_LINKS] = (unsigned long long)t0;
        acc[FEED_ACC_PATH] = (unsigned long long)t1; acc[FEED_ACC_LINK] = (unsigned long long)t2;
    }
}

/* third phase, a thread per waypoint: t = (the slice's start + the sum ahead of it on the slice) 2^-30 */
__global__ void __launch_bounds__(PCON_T) k_feed_time_rows(int W, int first_kept, const long long *__restrict__ tloc, const long long *__restrict__ slice_t,
        ppp_feed_row *__restrict__ rows)
{
    const int w = blockIdx.x * PCON_T + threadIdx.x;
    if (w >= W) return;
    rows[w].t = (double)(slice_t[rows[w].slice - first_kept] + tloc[w]) * (1.0 / FEED_TIME_FIXED);
}

/* the waypoints by limit and the extremes of the feed: integer atomics on counts and bit patterns, a wave, then one per wave,
   as k_dwell_stats counts */
__global__ void __launch_bounds__(PCON_T) k_feed_stats(const ppp_feed_row *__restrict__ rows, int W, unsigned long long *__restrict__ acc)
{
    unsigned long long cnt[4] = {0, 0, 0, 0}, mx = 0, nmn = 0;
    for (int w = blockIdx.x * PCON_T + threadIdx.x; w < W; w += gridDim.x * PCON_T) {
        const int l = rows[w].limit;
        const unsigned long long k = (unsigned long long)__double_as_longlong(rows[w].feed);
#pragma unroll
        for (int b = 0; b < 4; ++b) cnt[b] += l == b;
        mx = max(mx, k); nmn = max(nmn, ~k);
    }
#pragma unroll
    for (int b = 0; b < 4; ++b) cnt[b] = wave_sum(cnt[b]);
    mx = wave_max_bits(mx); nmn = wave_max_bits(nmn);
    if ((threadIdx.x & 63) == 0 && nmn) {
#pragma unroll
        for (int b = 0; b < 4; ++b) if (cnt[b]) atomicAdd(acc + FEED_ACC_LIMIT + b, cnt[b]);
        atomicMax(acc + FEED_ACC_MAX, mx); atomicMax(acc + FEED_ACC_NMIN, nmn);
    }
}
