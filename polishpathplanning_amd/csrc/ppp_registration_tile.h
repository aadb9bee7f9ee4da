/*
 * ppp_registration_tile.h -- point-to-plane registration of a scan held as slice-range tiles (ppp_get_registration_terms_tile,
 * ppp_merge_registration_terms, ppp_registration_step, ppp_register_tiles).  An evaluation is 29
 * integer sums over the scan's pairs, integer sums have no order, and the owned sets of ranges that tile the walk partition
 * the indexed points: the whole cloud's words are the word-by-word sum of the tiles'.  k_regt_terms is k_reg_terms over the
 * points a handle owns; the merge, the solve and the step run on the host with the routines the device chain runs
 * (icp_solve, icp_compose: __host__ __device__, and this unit is built with -ffp-contract=off on either side).
 * No float atomics.
 */
#pragma once
#include "ppp_registration.h"
#include <cstring>
#include <vector>

/* the words a tile's evaluation leaves: the 29 of the sums, the owned points it met, the owned queries that set the refusal */
#define REGT_OWNED ICP_WORDS
#define REGT_REFUSED (ICP_WORDS + 1)
#define REGT_WORDS (ICP_WORDS + 2)

/* What a slice-range reference must index around a moved query (B.89): [lo, hi] its indexed x interval, reach = 1.0001f *
   (max_dist + its normal_radius); check_lo / check_hi: the side is not the reference cloud's own end (leaves_indexed_range's
   exemption).  A whole-cloud reference checks neither side. */
struct RegtNeed {
    float lo, hi, reach;
    int check_lo, check_hi;
    __device__ inline bool refuses(float qx) const
    {
        return (check_lo && nextafterf(qx - reach, -INFINITY) < lo) || (check_hi && nextafterf(qx + reach, INFINITY) > hi);
    }
};

/* k_reg_terms for the positions [pos0, pos1) of the scan's index -- the slabs that meet the owned interval --, grid-stride: a
   position whose resident, unmoved x is not owned (B.36) is skipped; an owned point is moved by T (icp_move), the float of the
   moved point is paired in the slabs [rb0, rb1) the reference's handle sorted (dev_pair) and a pair adds its 29 terms
   (icp_add_terms); icp_flush.  An owned query with a finite moved position whose reach leaves what a slice-range reference
   indexes is counted in acc[REGT_REFUSED] and pairs with nothing: the host refuses the call.  T and the frame are read from
   device memory: the host writes T before every evaluation of the loop, the frame once. */
__global__ void __launch_bounds__(ICP_T) k_regt_terms(const float4 *__restrict__ q4, int pos0, int pos1, const TileRange own, const ContactIndex R,
        int nref, int rb0, int rb1, const RegtNeed need, const IcpFrame *__restrict__ Fp, const double *__restrict__ T,
        unsigned long long *__restrict__ acc)
{
    __shared__ unsigned long long s_a[ICP_T / 64][ICP_WORDS];
    __shared__ unsigned long long s_x[ICP_T / 64][2];
    const IcpFrame F = *Fp;
    unsigned long long a[ICP_WORDS];
#pragma unroll
    for (int w = 0; w < ICP_WORDS; ++w) a[w] = 0;
    unsigned long long mine = 0, refused = 0;
    double t[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) t[i] = T[i];
    for (int at = pos0 + blockIdx.x * ICP_T + threadIdx.x; at < pos1; at += gridDim.x * ICP_T) {
        const float4 p = q4[at];
        if (!own.owned(p.x)) continue;
        ++mine;
        double m[3];
        icp_move(t, p, m);
        const float qx = (float)m[0], qy = (float)m[1], qz = (float)m[2];
        if (!(isfinite(qx) && isfinite(qy) && isfinite(qz))) continue;
        if (need.refuses(qx)) { ++refused; continue; }
        DevPair P;
        if (dev_pair<false>(R, nref, rb0, rb1, qx, qy, qz, F.md2, P) != PPP_DEV_MATCHED) continue;
        icp_add_terms(a, m, P.q, P.n, F);
    }
    mine = wave_sum(mine); refused = wave_sum(refused);
    if ((threadIdx.x & 63) == 0) { s_x[threadIdx.x >> 6][0] = mine; s_x[threadIdx.x >> 6][1] = refused; }
    icp_flush<ICP_T>(a, s_a, acc); /* (its barrier stands between the stores above and the loads below) */
    if (threadIdx.x >= ICP_WORDS && threadIdx.x < REGT_WORDS) {
        unsigned long long s = 0;
        for (int v = 0; v < ICP_T / 64; ++v) s += s_x[v][threadIdx.x - ICP_WORDS];
        if (s) atomicAdd(acc + threadIdx.x, s);
    }
}

/* ---------------------------------------------------------------------------------------------------------------------- */
/* Host: the merge (B.91), the step (B.92) and the loop (B.93)                                                             */
/* ---------------------------------------------------------------------------------------------------------------------- */

/* do the parts belong to one evaluation of one scan against one reference?  n, shift, centre and length bit for bit */
inline bool regt_same_frame(const ppp_registration_part &a, const ppp_registration_part &b)
{
    return a.n == b.n && a.shift == b.shift && memcmp(a.centre, b.centre, sizeof(a.centre)) == 0 && memcmp(&a.length, &b.length, sizeof(double)) == 0;
}

/* B.92: reg_step_body's decision and arithmetic on a row whose transform is T: no step from fewer than 6 pairs, from six zero b
   (a stationary point) or from a solve that locks all six unknowns; else Tn, the mask and step2 */
inline int regt_step(const ppp_registration_row &row, const double *c, double Ln, double lock_eps, const double *T, double *Tn, int *locked,
                     double *step2)
{
    *locked = ICP_ALL_LOCKED; *step2 = icp_nan();
    if (row.pairs < 6) return PPP_STEP_FEW_PAIRS;
    bool zero = true;
    for (int i = 0; i < 6; ++i) zero = zero && row.b[i] == 0;
    if (zero) return PPP_STEP_STATIONARY;
    double x[6];
    const int mask = icp_solve(row.A, row.b, lock_eps, x);
    if (mask == ICP_ALL_LOCKED) return PPP_STEP_ALL_LOCKED;
    *step2 = icp_compose(x, c, Ln, T, Tn);
    *locked = mask;
    return PPP_STEP_TAKEN;
}

/* The host's loop of both tiled registrations (B.93): reg_step_body's control flow, word for word -- `stop` behind a step below
   min_step makes the next evaluation the last, an evaluation no step is taken from ends the loop, and the evaluation behind the
   last of `iterations` steps is a row without a step.  eval(k, rw): evaluation k at T, merged over the tiles, or its error. */
template <typename Eval>
inline int regt_loop(const ppp_registration_params &P, const IcpFrame &F, double *T, std::vector<ppp_registration_row> &R, IcpCtl &C,
                     ppp_registration_part &whole, Eval eval)
{
    for (int k = 0; k <= P.iterations; ++k) {
        ppp_registration_row rw;
        const int rc = eval(k, rw);
        if (rc) return rc;
        if (k == P.iterations) { R.push_back(rw); break; } /* the evaluation behind the last step */
        double Tn[12];
        int mask = ICP_ALL_LOCKED;
        double step2 = icp_nan();
        if (!C.stop) {
            const int sc = regt_step(rw, whole.centre, whole.length, F.lock_eps, T, Tn, &mask, &step2);
            if (sc == PPP_STEP_STATIONARY) C.converged = 1;
        }
        if (mask == ICP_ALL_LOCKED) { R.push_back(rw); C.done = 1; break; }
        rw.locked = mask; rw.step2 = step2;
        R.push_back(rw);
        C.steps += 1; C.locked |= mask;
        if (step2 < F.min_step2) { C.stop = 1; C.converged = 1; }
        memcpy(T, Tn, 12 * sizeof(double));
    }
    return PPP_OK;
}
