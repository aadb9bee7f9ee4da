/*
 * ppp_registration.h -- point-to-plane ICP of one handle's cloud, the scan, to another handle's, the reference
 * (ppp_get_registration_terms, ppp_register).  An iteration is k_reg_terms -- the scan's points, moved
 * by the current transform, through the reference's slab index (dev_nearest_within and k_dev_nearest's pair rule) and the 29
 * integer sums of the normal equations -- and k_reg_step, one thread that solves the 6 x 6 system and composes the next
 * transform.  The transforms, the sums and the rows stay on the device: the host enqueues the whole chain and waits once.
 * Integer sums wherever a sum has no order, + - * / in double with one rounding per written operation everywhere else: the
 * same bits in every run.  No float atomics, no transcendental on the path that decides anything.
 * Global registration (ppp_get_cloud_moments, ppp_register_global): k_cloud_moments, the ten integer
 * words of a cloud's first and second moments; cloud_frame_from_words, the principal frame they imply, and registration_starts,
 * the rigid motions two such frames imply (host); k_reg_terms_multi and k_reg_step_multi, K chains side by side -- start
 * blockIdx.y of the evaluation, workgroup blockIdx.x of the step -- on the queries StrideSel compacts once.
 */
#pragma once
#include "ppp_deviation.h"
#include "ppp_compact.h"

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

/* m = T p in double: ((t0 px + t1 py) + t2 pz) + t3 per row, one rounding per written operation */
__device__ __attribute__((always_inline)) inline void icp_move(const double *t, const float4 &p, double *m)
{
    const double px = (double)p.x, py = (double)p.y, pz = (double)p.z;
#pragma unroll
    for (int r = 0; r < 3; ++r) m[r] = ((t[4 * r] * px + t[4 * r + 1] * py) + t[4 * r + 2] * pz) + t[4 * r + 3];
}

/* a pair's 29 terms -- the moved point m, its partner q with the normal n -- each rounded to 2^-shift (F.scale = 2^shift), added
   to the thread's 64-bit integers a.  Two's complement words: b may be negative. */
__device__ __attribute__((always_inline)) inline void icp_add_terms(unsigned long long *a, const double *m, const float4 &q, const float4 &n,
                                                                   const IcpFrame &F)
{
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

/* the same 29 terms for a partner and a normal that are doubles already (k_mesh_reg_terms: the closest point on a triangle and
   the facet's own normal): the float4 form's expressions, operation for operation, without its widening casts */
__device__ __attribute__((always_inline)) inline void icp_add_terms(unsigned long long *a, const double *m, const double *q, const double *n,
                                                                   const IcpFrame &F)
{
    const double nx = n[0], ny = n[1], nz = n[2];
    const double ex = m[0] - q[0], ey = m[1] - q[1], ez = m[2] - q[2];
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

/* the threads' words of a workgroup of T threads into acc: over the wave, over the workgroup through LDS, and one 64-bit
   integer atomic per non-zero word */
template <int T>
__device__ __attribute__((always_inline)) inline void icp_flush(unsigned long long *a, unsigned long long (*s_a)[ICP_WORDS],
                                                               unsigned long long *__restrict__ acc)
{
#pragma unroll
    for (int w = 0; w < ICP_WORDS; ++w) a[w] = wave_sum(a[w]);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int w = 0; w < ICP_WORDS; ++w) s_a[threadIdx.x >> 6][w] = a[w];
    }
    __syncthreads();
    if (threadIdx.x < ICP_WORDS) {
        unsigned long long s = 0;
        for (int v = 0; v < T / 64; ++v) s += s_a[v][threadIdx.x];
        if (s) atomicAdd(acc + threadIdx.x, s);
    }
}

/* The hot path (B.69): a thread per indexed point of the scan, in the scan's slab order (q4 = its sorted4, nq = its n_sorted),
   grid-stride.  The point is moved by T in double (icp_move), the float of the moved point is searched in the reference's whole
   index R (dev_nearest_within<true>) and paired by dev_pair's rule -- written out here, not called: with the pair handed back as
   dev_pair's record this kernel came to 155 - 157 VGPRs for 148 and ran 0.4 - 1.2 % slower in ppp_register's chains
   (profiles/scan_reference_fold_ab.txt); k_trim_pair, which calls dev_pair, is compared with it bit for bit at keep = 1 -- and a
   pair adds its 29 terms (icp_add_terms).  icp_flush: the grid is capped by the host, so the atomics do not grow with the
   cloud.  T is read from device memory -- the step kernel before this launch wrote it. */
/* k_reg_terms's body, for workgroup `block` of `blocks`: one chain's evaluation at T into acc.  Both the single chain's kernel
   and the side-by-side one call it, so a row is the same bits from either. */
__device__ __forceinline__ void reg_terms_body(const float4 *__restrict__ q4, int nq, const ContactIndex &R, int nref, const IcpFrame &F,
        const double *__restrict__ T, unsigned long long *__restrict__ acc, int block, int blocks)
{
    __shared__ unsigned long long s_a[ICP_T / 64][ICP_WORDS];
    unsigned long long a[ICP_WORDS];
#pragma unroll
    for (int w = 0; w < ICP_WORDS; ++w) a[w] = 0;
    double t[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) t[i] = T[i];
    for (int at = block * ICP_T + threadIdx.x; at < nq; at += blocks * ICP_T) {
        double m[3];
        icp_move(t, q4[at], m);
        const float qx = (float)m[0], qy = (float)m[1], qz = (float)m[2];
        if (!(isfinite(qx) && isfinite(qy) && isfinite(qz)) || nref <= 0) continue;
        float4 q = make_float4(NAN, NAN, NAN, 0.f);
        float dd = NAN;
        const int j = dev_nearest_within<true>(R.view(), 0, 0, qx, qy, qz, F.md2, &q, &dd);
        if (j < 0) continue;
        const float4 n = R.normals4[j];
        if (!(n.x == n.x && n.y == n.y && n.z == n.z && n.w == n.w)) continue;
        icp_add_terms(a, m, q, n, F);
    }
    icp_flush<ICP_T>(a, s_a, acc);
}

__global__ void __launch_bounds__(ICP_T) k_reg_terms(const float4 *__restrict__ q4, int nq, const ContactIndex R, int nref, const IcpFrame F,
        const double *__restrict__ T, const IcpCtl *__restrict__ ctl, unsigned long long *__restrict__ acc)
{
    if (ctl->done) return;
    reg_terms_body(q4, nq, R, nref, F, T, acc, blockIdx.x, gridDim.x);
}

/* K chains side by side (B.76): start blockIdx.y evaluates at its own transform into its own 29 words -- T, acc and ctl are
   those of start 0, a start's lie tstride doubles, astride words and one IcpCtl behind its predecessor's -- with gridDim.x
   workgroups striding over the nq queries, so the lanes of a workgroup walk the same windows of the reference's index.  A
   chain that has ended returns at its first instruction, whatever the others do. */
__global__ void __launch_bounds__(ICP_T) k_reg_terms_multi(const float4 *__restrict__ q4, int nq, const ContactIndex R, int nref, const IcpFrame F,
        const double *__restrict__ T, size_t tstride, const IcpCtl *__restrict__ ctl, unsigned long long *__restrict__ acc, size_t astride)
{
    if (ctl[blockIdx.y].done) return;
    reg_terms_body(q4, nq, R, nref, F, T + blockIdx.y * tstride, acc + blockIdx.y * astride, blockIdx.x, gridDim.x);
}

/* One thread: the evaluation k of a chain (its 29 words in acc, its transform T) becomes row k, and, where a step is taken
   from it, T + 12 the next transform.  No step is taken -- the row keeps locked = 63 and step2 = NaN and the chain ends --
   behind a step below min_step (ctl->stop: converged), where J^T r is zero in every word (T is a stationary point: converged),
   with fewer than 6 pairs, and where the pivot rule locks all six unknowns (not converged). */
__device__ __forceinline__ void reg_step_body(const unsigned long long *__restrict__ acc, const IcpFrame &F, double *T,
        ppp_registration_row *__restrict__ row, IcpCtl *ctl)
{
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

__global__ void __launch_bounds__(64) k_reg_step(const unsigned long long *__restrict__ acc, const IcpFrame F, double *T,
        ppp_registration_row *__restrict__ row, IcpCtl *ctl)
{
    if (ctl->done || threadIdx.x != 0 || blockIdx.x != 0) return;
    reg_step_body(acc, F, T, row, ctl);
}

/* the steps of K chains: workgroup blockIdx.x is start blockIdx.x, in which thread 0 works; the strides are k_reg_terms_multi's,
   rstride rows lie between two starts' */
__global__ void __launch_bounds__(64) k_reg_step_multi(const unsigned long long *__restrict__ acc, size_t astride, const IcpFrame F, double *T,
        size_t tstride, ppp_registration_row *__restrict__ row, size_t rstride, IcpCtl *ctl)
{
    const size_t s = blockIdx.x;
    if (ctl[s].done || threadIdx.x != 0) return;
    reg_step_body(acc + s * astride, F, T + s * tstride, row + s * rstride, ctl + s);
}

/* The coarse stage's queries (B.76): the indexed points of the scan whose cloud index is a multiple of stride, in slab order */
struct StrideSel {
    using Val = float4;
    const float4 *q4;
    int stride;
    float4 *out;
    __device__ void begin() {}
    __device__ float4 load(int i) const { return q4[i]; }
    __device__ bool keep(int, const float4 &p) const { return idx_of(p) % stride == 0; }
    __device__ void emit(int, int k, const float4 &p) const { out[k] = p; }
};

/* ---------------------------------------------------------------------------------------------------------------------- */
/* The principal frame of a cloud (B.73, B.74) and the starts two frames imply (B.75)                                     */
/* ---------------------------------------------------------------------------------------------------------------------- */
#define MOM_T 256
#define MOM_WORDS 10 /* the count, S1[x y z], S2[xx xy xz yy yz zz] */
#define MOM_SWEEPS 12

struct MomFrame { double c[3], L, scale; };

/* B.73: min(40, 60 - clog2(max(2, n))), n = cloud->size() */
__host__ __device__ inline int mom_shift(size_t n)
{
    const int s = 60 - icp_clog2((double)(n < 2 ? (size_t)2 : n));
    return s < 40 ? s : 40;
}

/* the threads' ten words of a workgroup of MOM_T threads into acc: icp_flush's pattern (k_cloud_moments, k_mesh_moments) */
__device__ __attribute__((always_inline)) inline void mom_flush(unsigned long long *a, unsigned long long (*s_a)[MOM_WORDS],
                                                               unsigned long long *__restrict__ acc)
{
#pragma unroll
    for (int w = 0; w < MOM_WORDS; ++w) a[w] = wave_sum(a[w]);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int w = 0; w < MOM_WORDS; ++w) s_a[threadIdx.x >> 6][w] = a[w];
    }
    __syncthreads();
    if (threadIdx.x < MOM_WORDS) {
        unsigned long long s = 0;
        for (int v = 0; v < MOM_T / 64; ++v) s += s_a[v][threadIdx.x];
        if (s) atomicAdd(acc + threadIdx.x, s);
    }
}

/* A thread per indexed point in slab order, grid-stride: u = ((double)p - c) / L, the ten words rounded to 2^-ms (F.scale =
   2^ms) into the thread's 64-bit integers, added over the wave, over the workgroup through LDS, and by one 64-bit integer
   atomic per workgroup and non-zero word: k_reg_terms's pattern.  |u_d| <= 1 and n 2^ms <= 2^60: no word overflows. */
__global__ void __launch_bounds__(MOM_T) k_cloud_moments(const float4 *__restrict__ q4, int nq, const MomFrame F, unsigned long long *__restrict__ acc)
{
    __shared__ unsigned long long s_a[MOM_T / 64][MOM_WORDS];
    unsigned long long a[MOM_WORDS];
#pragma unroll
    for (int w = 0; w < MOM_WORDS; ++w) a[w] = 0;
    for (int at = blockIdx.x * MOM_T + threadIdx.x; at < nq; at += gridDim.x * MOM_T) {
        const float4 p = q4[at];
        const double u[3] = {((double)p.x - F.c[0]) / F.L, ((double)p.y - F.c[1]) / F.L, ((double)p.z - F.c[2]) / F.L};
        a[0] += 1;
        int w = 4;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            a[1 + d] += (unsigned long long)llrint(u[d] * F.scale);
#pragma unroll
            for (int k = d; k < 3; ++k, ++w) a[w] += (unsigned long long)llrint((u[d] * u[k]) * F.scale);
        }
    }
    mom_flush(a, s_a, acc);
}

/* B.74 behind the mean m and the covariance A of u (A is used up): the eigenpairs by MOM_SWEEPS cyclic Jacobi sweeps over the
   pairs (0,1), (0,2), (1,2) -- a pair whose off-diagonal entry is zero is skipped; theta = (a_qq - a_pp) / (2 a_pq),
   t = sgn(theta) / (|theta| + sqrt(theta theta + 1)), c = 1 / sqrt(t t + 1), s = t c; a_pp -= t a_pq, a_qq += t a_pq, a_pq = 0,
   the third index r: (a_rp, a_rq) <- (c a_rp - s a_rq, s a_rp + c a_rq), every row k of V likewise -- + - * / and sqrt, one
   rounding per written operation; eigenvalues descending, a tie to the lower original column; the first two axes signed so
   that the component of largest magnitude is positive (the lowest index on a tie), the third their cross product; mean =
   c + L m, eigenvalues = (lambda L) L.  Both the points' frame (cloud_frame_from_words) and the surface's
   (mesh_frame_from_words, ppp_mesh_registration.h) end here. */
inline void frame_from_mean_cov(const double *m, double (*A)[3], const double *c, double L, ppp_cloud_frame *f)
{
    double V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    static const int PQ[3][3] = {{0, 1, 2}, {0, 2, 1}, {1, 2, 0}};
    for (int sweep = 0; sweep < MOM_SWEEPS; ++sweep)
        for (int e = 0; e < 3; ++e) {
            const int p = PQ[e][0], q = PQ[e][1], r = PQ[e][2];
            const double apq = A[p][q];
            if (apq == 0.0) continue;
            const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
            const double at = theta < 0.0 ? -theta : theta;
            const double den = at + std::sqrt(theta * theta + 1.0);
            const double t = theta < 0.0 ? -1.0 / den : 1.0 / den;
            const double cs = 1.0 / std::sqrt(t * t + 1.0), sn = t * cs;
            A[p][p] = A[p][p] - t * apq;
            A[q][q] = A[q][q] + t * apq;
            A[p][q] = A[q][p] = 0.0;
            const double arp = A[r][p], arq = A[r][q];
            A[r][p] = A[p][r] = cs * arp - sn * arq;
            A[r][q] = A[q][r] = sn * arp + cs * arq;
            for (int k = 0; k < 3; ++k) {
                const double vp = V[k][p], vq = V[k][q];
                V[k][p] = cs * vp - sn * vq;
                V[k][q] = sn * vp + cs * vq;
            }
        }
    int ord[3] = {0, 1, 2}; /* descending, stable: a tie keeps the lower original column first */
    for (int i = 1; i < 3; ++i)
        for (int k = i; k > 0 && A[ord[k]][ord[k]] > A[ord[k - 1]][ord[k - 1]]; --k) { const int o = ord[k]; ord[k] = ord[k - 1]; ord[k - 1] = o; }
    double ax[3][3]; /* ax[k] = axis k */
    for (int k = 0; k < 2; ++k) {
        int big = 0;
        for (int d = 1; d < 3; ++d) if (std::fabs(V[d][ord[k]]) > std::fabs(V[big][ord[k]])) big = d;
        const bool neg = V[big][ord[k]] < 0.0;
        for (int d = 0; d < 3; ++d) ax[k][d] = neg ? -V[d][ord[k]] : V[d][ord[k]];
    }
    ax[2][0] = ax[0][1] * ax[1][2] - ax[0][2] * ax[1][1];
    ax[2][1] = ax[0][2] * ax[1][0] - ax[0][0] * ax[1][2];
    ax[2][2] = ax[0][0] * ax[1][1] - ax[0][1] * ax[1][0];
    for (int d = 0; d < 3; ++d) {
        f->mean[d] = c[d] + L * m[d];
        f->eigenvalues[d] = (A[ord[d]][ord[d]] * L) * L;
        for (int k = 0; k < 3; ++k) f->axes[3 * d + k] = ax[k][d];
    }
}

/* B.74: the frame the ten words of a cloud's points imply: mean and covariance of u in double, then frame_from_mean_cov.
   false: no point, or L not finite and > 0. */
inline bool cloud_frame_from_words(const long long *words, int ms, const double *c, double L, ppp_cloud_frame *f)
{
    if (words[0] <= 0 || !(L > 0.0) || !(L < INFINITY) || ms < 0 || ms > 62) return false;
    f->count = (size_t)words[0]; f->ms = ms; f->L = L;
    for (int d = 0; d < 3; ++d) f->c[d] = c[d];
    for (int w = 0; w < MOM_WORDS; ++w) f->words[w] = words[w];
    double inv = 1.0;
    for (int i = 0; i < ms; ++i) inv = inv * 0.5; /* 2^-ms */
    const double cnt = (double)words[0];
    double m[3], A[3][3];
    for (int d = 0; d < 3; ++d) m[d] = ((double)words[1 + d] / cnt) * inv;
    for (int d = 0, w = 4; d < 3; ++d)
        for (int k = d; k < 3; ++k, ++w) A[d][k] = A[k][d] = ((double)words[w] / cnt) * inv - m[d] * m[k];
    frame_from_mean_cov(m, A, c, L, f);
    return true;
}

/* B.75: the proper signed permutations G in their fixed order -- column k of G has the entry sgn[k] in row perm[k] -- the
   identity, the half turns about the first, the second and the third axis, then the other 20 ascending in (perm[0], perm[1],
   perm[2], sgn[0], sgn[1], sgn[2]) with + before - */
struct StartG { int perm[3], sgn[3]; };
inline void registration_start_table(StartG *G)
{
    static const int P[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
    static const int PAR[6] = {1, -1, -1, 1, 1, -1};
    static const int HEAD[4][3] = {{1, 1, 1}, {1, -1, -1}, {-1, 1, -1}, {-1, -1, 1}};
    int n = 0;
    for (int i = 0; i < 4; ++i, ++n)
        for (int k = 0; k < 3; ++k) { G[n].perm[k] = k; G[n].sgn[k] = HEAD[i][k]; }
    for (int p = 0; p < 6; ++p)
        for (int b = 0; b < 8; ++b) {
            const int s[3] = {(b & 4) ? -1 : 1, (b & 2) ? -1 : 1, (b & 1) ? -1 : 1};
            if (PAR[p] * s[0] * s[1] * s[2] != 1 || p == 0) continue;
            for (int k = 0; k < 3; ++k) { G[n].perm[k] = P[p][k]; G[n].sgn[k] = s[k]; }
            ++n;
        }
}

/* T12s[12 g ..] = (R_G | t_G): R_G = (V_ref G) V_scan^T, t_G = mean_ref - R_G mean_scan, every sum ((a0 b0) + a1 b1) + a2 b2 */
inline void registration_starts(const ppp_cloud_frame *scan, const ppp_cloud_frame *ref, int candidates, double *T12s)
{
    StartG G[24];
    registration_start_table(G);
    for (int g = 0; g < candidates; ++g) {
        double *T = T12s + 12 * g;
        for (int r = 0; r < 3; ++r) {
            double a[3];
            for (int k = 0; k < 3; ++k) { const double v = ref->axes[3 * r + G[g].perm[k]]; a[k] = G[g].sgn[k] < 0 ? -v : v; }
            for (int cc = 0; cc < 3; ++cc) T[4 * r + cc] = ((a[0] * scan->axes[3 * cc]) + a[1] * scan->axes[3 * cc + 1]) + a[2] * scan->axes[3 * cc + 2];
            T[4 * r + 3] = ref->mean[r] - (((T[4 * r] * scan->mean[0]) + T[4 * r + 1] * scan->mean[1]) + T[4 * r + 2] * scan->mean[2]);
        }
    }
}
