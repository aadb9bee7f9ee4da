/*
 * ppp_registration.h -- point-to-plane ICP of one handle's cloud, the scan, to another handle's, the reference
 * (ppp_get_registration_terms, ppp_register).  An iteration is k_reg_terms -- the scan's points, moved
 * by the current transform, through the reference's slab index (dev_nearest_within, as k_dev_nearest walks it) and the 29
 * integer sums of the normal equations -- and k_reg_step, one thread that solves the 6 x 6 system and composes the next
 * transform.  The transforms, the sums and the rows stay on the device: the host enqueues the whole chain and waits once.
 * Integer sums wherever a sum has no order, + - * / in double with one rounding per written operation everywhere else: the
 * same bits in every run.  No float atomics, no transcendental on the path that decides anything.
 */
#pragma once
#include "ppp_deviation.h"

#define ICP_T 256
#define ICP_PAIRS 0  /* the words of one evaluation: pairs, the upper triangle of J^T J (21), J^T r (6), r^T r */
#define ICP_A 1
#define ICP_B 22
#define ICP_E 28
#define ICP_WORDS 29
#define ICP_ALL_LOCKED 63

/* what does not change along a chain: the centre and the length that scale the rotation's unknowns (B.67), 2^shift, the
   float bound of the search, and the solve's and the loop's parameters */
struct IcpFrame {
    double c[3], Ln, scale;
    double lock_eps, min_step2;
    float md2;
};

/* the words a chain's step kernels leave for each other and for the host */
struct IcpCtl {
    int done;       /* the chain has ended: every later kernel returns at once */
    int stop;       /* the step just taken was below min_step: the next evaluation is the last */
    int steps, converged, locked;
};

/* the smallest e with 2^e >= x (x >= 1, finite) */
__host__ __device__ inline int icp_clog2(double x)
{
    int e = 0;
    for (double p = 1.0; p < x; p *= 2.0) ++e;
    return e;
}

/* B.68: min(40, 60 - clog2(max(2, n)) - clog2(max(1, ceil(md2)))), md2 the float product max_dist * max_dist (finite) */
__host__ __device__ inline int icp_shift(size_t n, float md2)
{
    const double m = ceil((double)md2);
    const int s = 60 - icp_clog2((double)(n < 2 ? (size_t)2 : n)) - icp_clog2(m < 1.0 ? 1.0 : m);
    return s < 40 ? s : 40;
}

/* the quiet NaN of a row that no step was taken from: one bit pattern, so rows compare as bytes */
__host__ __device__ inline double icp_nan()
{
    const unsigned long long u = 0x7ff8000000000000ull;
    double d; __builtin_memcpy(&d, &u, 8);
    return d;
}

/* row <- the evaluation at T (its transform and its 29 words), as a row that no step was taken from */
__host__ __device__ inline void icp_row_terms(ppp_registration_row *row, const double *T, const unsigned long long *acc)
{
    for (int i = 0; i < 12; ++i) row->T[i] = T[i];
    row->pairs = (size_t)acc[ICP_PAIRS];
    for (int i = 0; i < 21; ++i) row->A[i] = (long long)acc[ICP_A + i];
    for (int i = 0; i < 6; ++i) row->b[i] = (long long)acc[ICP_B + i];
    row->E = (long long)acc[ICP_E];
    row->locked = ICP_ALL_LOCKED;
    row->step2 = icp_nan();
}

/* B.70: LDL^T of M = (double)A in index order with the pivot rule -- unknown i is locked (x_i = 0, no part in any later sum)
   unless v_i > lock_eps * the largest M_ii -- and the two substitutions for g = -(double)b.  Every sum runs over the unlocked k
   in ascending order, starts at 0 and is subtracted whole.  Returns the mask of the locked unknowns. */
__host__ __device__ inline int icp_solve(const long long *A, const long long *b, double lock_eps, double *x)
{
    double M[6][6], L[6][6], d[6], g[6], z[6];
    for (int i = 0, w = 0; i < 6; ++i)
        for (int k = i; k < 6; ++k, ++w) M[i][k] = M[k][i] = (double)A[w];
    double big = M[0][0];
    for (int i = 1; i < 6; ++i) if (M[i][i] > big) big = M[i][i];
    const double floor_v = lock_eps * big;
    int locked = 0;
    for (int i = 0; i < 6; ++i) {
        g[i] = -(double)b[i];
        d[i] = 0.0; z[i] = 0.0; x[i] = 0.0;
        for (int k = 0; k < 6; ++k) L[i][k] = 0.0;
    }
    for (int i = 0; i < 6; ++i) {
        double s = 0.0;
        for (int k = 0; k < i; ++k) if (!((locked >> k) & 1)) s = s + (L[i][k] * L[i][k]) * d[k];
        const double v = M[i][i] - s;
        if (!(v > floor_v)) { locked |= 1 << i; continue; }
        d[i] = v;
        for (int j = i + 1; j < 6; ++j) {
            double t = 0.0;
            for (int k = 0; k < i; ++k) if (!((locked >> k) & 1)) t = t + (L[j][k] * L[i][k]) * d[k];
            L[j][i] = (M[j][i] - t) / v;
        }
    }
    for (int i = 0; i < 6; ++i) { /* L z = g */
        if ((locked >> i) & 1) continue;
        double s = 0.0;
        for (int k = 0; k < i; ++k) if (!((locked >> k) & 1)) s = s + L[i][k] * z[k];
        z[i] = g[i] - s;
    }
    for (int i = 5; i >= 0; --i) { /* L^T x = D^-1 z */
        if ((locked >> i) & 1) continue;
        double s = 0.0;
        for (int k = i + 1; k < 6; ++k) if (!((locked >> k) & 1)) s = s + L[k][i] * x[k];
        x[i] = z[i] / d[i] - s;
    }
    return locked;
}

/* B.71: the step x as a rigid motion about c -- the rotation in Cayley's form, built without a transcendental -- composed
   with T: Tn = (dR R | (dR (t - c) + c) + dt).  Returns step2. */
__host__ __device__ inline double icp_compose(const double *x, const double *c, double Ln, const double *T, double *Tn)
{
    const double hx = (x[0] / Ln) * 0.5, hy = (x[1] / Ln) * 0.5, hz = (x[2] / Ln) * 0.5;
    const double s = (hx * hx + hy * hy) + hz * hz;
    const double den = 1.0 + s, dg = 1.0 - s;
    double dR[3][3];
    dR[0][0] = (dg + 2.0 * (hx * hx)) / den;
    dR[1][1] = (dg + 2.0 * (hy * hy)) / den;
    dR[2][2] = (dg + 2.0 * (hz * hz)) / den;
    dR[0][1] = (2.0 * (hx * hy) - 2.0 * hz) / den; dR[1][0] = (2.0 * (hy * hx) + 2.0 * hz) / den;
    dR[0][2] = (2.0 * (hx * hz) + 2.0 * hy) / den; dR[2][0] = (2.0 * (hz * hx) - 2.0 * hy) / den;
    dR[1][2] = (2.0 * (hy * hz) - 2.0 * hx) / den; dR[2][1] = (2.0 * (hz * hy) + 2.0 * hx) / den;
    const double d0 = T[3] - c[0], d1 = T[7] - c[1], d2 = T[11] - c[2];
    for (int r = 0; r < 3; ++r) {
        for (int k = 0; k < 3; ++k) Tn[4 * r + k] = ((dR[r][0] * T[k]) + dR[r][1] * T[4 + k]) + dR[r][2] * T[8 + k];
        Tn[4 * r + 3] = ((((dR[r][0] * d0) + dR[r][1] * d1) + dR[r][2] * d2) + c[r]) + x[3 + r];
    }
    const double rot = (x[0] * x[0] + x[1] * x[1]) + x[2] * x[2], tr = (x[3] * x[3] + x[4] * x[4]) + x[5] * x[5];
    return rot > tr ? rot : tr;
}

/* The hot path (B.69): a thread per indexed point of the scan, in the scan's slab order (q4 = its sorted4, nq = its n_sorted),
   grid-stride.  The point is moved by T in double, the float of the moved point is searched in the reference's index R with
   k_dev_nearest's walk and rule, and a pair adds its 29 terms, each rounded to 2^-shift (F.scale = 2^shift), to the thread's
   64-bit integers.  They are added over the wave, over the workgroup through LDS, and the workgroup adds every non-zero word
   with one 64-bit integer atomic: the grid is capped by the host, so the atomics do not grow with the cloud.  Two's complement
   words: b may be negative.  T is read from device memory -- the step kernel before this launch wrote it. */
__global__ void __launch_bounds__(ICP_T) k_reg_terms(const float4 *__restrict__ q4, int nq, const ContactIndex R, int nref, const IcpFrame F,
        const double *__restrict__ T, const IcpCtl *__restrict__ ctl, unsigned long long *__restrict__ acc)
{
    if (ctl->done) return;
    __shared__ unsigned long long s_a[ICP_T / 64][ICP_WORDS];
    unsigned long long a[ICP_WORDS];
#pragma unroll
    for (int w = 0; w < ICP_WORDS; ++w) a[w] = 0;
    double t[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) t[i] = T[i];
    const SlabView V = R.view();
    for (int at = blockIdx.x * ICP_T + threadIdx.x; at < nq; at += gridDim.x * ICP_T) {
        const float4 p = q4[at];
        const double px = (double)p.x, py = (double)p.y, pz = (double)p.z;
        double m[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) m[r] = ((t[4 * r] * px + t[4 * r + 1] * py) + t[4 * r + 2] * pz) + t[4 * r + 3];
        const float qx = (float)m[0], qy = (float)m[1], qz = (float)m[2];
        if (!(isfinite(qx) && isfinite(qy) && isfinite(qz)) || nref <= 0) continue;
        float4 q = make_float4(NAN, NAN, NAN, 0.f);
        float dd = NAN;
        const int j = dev_nearest_within(V, qx, qy, qz, F.md2, &q, &dd);
        if (j < 0) continue;
        const float4 n = R.normals4[j];
        if (!(n.x == n.x && n.y == n.y && n.z == n.z && n.w == n.w)) continue;
        const double nx = (double)n.x, ny = (double)n.y, nz = (double)n.z;
        const double ex = m[0] - (double)q.x, ey = m[1] - (double)q.y, ez = m[2] - (double)q.z;
        const double r = ((ex * nx) + ey * ny) + ez * nz;
        const double ux = (m[0] - F.c[0]) / F.Ln, uy = (m[1] - F.c[1]) / F.Ln, uz = (m[2] - F.c[2]) / F.Ln;
        const double J[6] = {uy * nz - uz * ny, uz * nx - ux * nz, ux * ny - uy * nx, nx, ny, nz};
        a[ICP_PAIRS] += 1;
        int w = ICP_A;
#pragma unroll
        for (int i = 0; i < 6; ++i) {
#pragma unroll
            for (int k = i; k < 6; ++k, ++w) a[w] += (unsigned long long)llrint((J[i] * J[k]) * F.scale);
            a[ICP_B + i] += (unsigned long long)llrint((J[i] * r) * F.scale);
        }
        a[ICP_E] += (unsigned long long)llrint((r * r) * F.scale);
    }
#pragma unroll
    for (int w = 0; w < ICP_WORDS; ++w) a[w] = wave_sum(a[w]);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int w = 0; w < ICP_WORDS; ++w) s_a[threadIdx.x >> 6][w] = a[w];
    }
    __syncthreads();
    if (threadIdx.x < ICP_WORDS) {
        unsigned long long s = 0;
        for (int v = 0; v < ICP_T / 64; ++v) s += s_a[v][threadIdx.x];
        if (s) atomicAdd(acc + threadIdx.x, s);
    }
}

/* One thread: the evaluation k of a chain (its 29 words in acc, its transform T) becomes row k, and, where a step is taken
   from it, T + 12 the next transform.  No step is taken -- the row keeps locked = 63 and step2 = NaN and the chain ends --
   behind a step below min_step (ctl->stop: converged), where J^T r is zero in every word (T is a stationary point: converged),
   with fewer than 6 pairs, and where the pivot rule locks all six unknowns (not converged). */
__global__ void __launch_bounds__(64) k_reg_step(const unsigned long long *__restrict__ acc, const IcpFrame F, double *T,
        ppp_registration_row *__restrict__ row, IcpCtl *ctl)
{
    if (ctl->done || threadIdx.x != 0 || blockIdx.x != 0) return;
    ppp_registration_row rw;
    icp_row_terms(&rw, T, acc);
    bool zero = true;
    for (int i = 0; i < 6; ++i) zero = zero && rw.b[i] == 0;
    double x[6];
    int mask = ICP_ALL_LOCKED;
    if (!ctl->stop && rw.pairs >= 6) {
        if (zero) ctl->converged = 1;
        else mask = icp_solve(rw.A, rw.b, F.lock_eps, x);
    }
    if (mask == ICP_ALL_LOCKED) { *row = rw; ctl->done = 1; return; }
    rw.step2 = icp_compose(x, F.c, F.Ln, T, T + 12);
    rw.locked = mask;
    *row = rw;
    ctl->steps += 1;
    ctl->locked |= mask;
    if (rw.step2 < F.min_step2) { ctl->stop = 1; ctl->converged = 1; }
}
