// ltp_stop.hip — stop plans (ltp_plan_stop_batch, include/ltp_hip.h): every joint of every query brakes to rest by optBraking
// (cc:650-701), gfx950. A translation unit of its own: the code objects of the stage, sampler and consumer kernels do not depend on it.
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (see Makefile), no fast-math, like the stage kernels.
#include "ltp_device.hpp"

namespace ltp {

// Block = 64 queries x JB joint slots, k_opt_fast's shape: wave y handles joints y, y + JB, ... of 64 consecutive queries. No new
// arithmetic: check_inputs_joint, opt_braking, cumsum7 and joint_len are the functions the stage kernels and the one-lane mirrors call.
//   pass 1  the chosen check per (query, joint); a query is rejected when any joint fails (needed before anything is stored: a rejected
//           query's t_scaled is zero, and with dof > JB its joints are spread over several rounds)
//   pass 2  per round of JB joints, optBraking per (query, joint): t_opt = t_scaled = cumsum(t_rel), dir, mod 0, v_drive = v_max,
//           q_stop = q_0 + q; each wave keeps the slowest of its joints (ascending j, strict '>': the first one wins, NaN never),
//           lengths fold into LDS
//   then    per query: the waves' candidates in slot order with ties to the smaller joint (cc:31-39), t_required, slowest, traj_len
//           (cc:716-719) and status, so that launch_offsets(..., lens_ready = true) follows without reading t_scaled again
// A rejected query keeps t_opt / dir / t_required / slowest (what ltp_plan_switch_times_batch leaves for it when it is planned towards
// the standstill position: k_opt_fast stores stage 1 whatever checkInputs says) and gets t_scaled 0, traj_len 0 and NaN in q_stop; a
// bad set index gets the zero record k_opt_fast / k_reduce_scale leave.
// The limits come through plan_limits() with or without a binding: one instantiation per pow rule.
//
// Stores. A lane's record is 56 + 56 + 8 + 8 + 1 bytes at a lane stride of dof * 56 (dof * 8, dof) bytes: stored per lane, every
// store instruction of a wave touches 64 lines. So the round's records go through LDS instead and leave as consecutive 8-byte
// elements — the round's joints [jb, jb + nj) of the block's queries are nq runs of nj * 7 (nj, nj) elements, ONE run when
// dof <= JB — and a wave's store instruction covers 512 consecutive bytes. Measured (profiles/r18_stop.txt): the
// per-lane form was 19-24 % slower and is gone; c4ff620 is the last commit that builds it (-DLTP_STOP_STAGED=0).
constexpr int kStopCheckBraking = 1;   // LTP_STOP_CHECK_BRAKING; anything else (the entry admits only 0) is LTP_STOP_CHECK_INPUTS

// elements [0, nq * nj * P) of the round's staging array s — lane (x, y) holds P elements at (x * nj + y) * P — to their places in the
// query-major record array dst: element e of query x at ((q_blk + x) * dof + jb) * P + e. Every thread of the block calls it.
template <int P, class T, class S, class F>
LTP_DEV void store_round(T* __restrict__ dst, const S* s, int nq, int nj, int dof, long long q_blk, int jb, F value)
{
    const int threads = (int)(blockDim.x * blockDim.y), tid = (int)(threadIdx.y * blockDim.x + threadIdx.x);
    const int run = nj * P, total = nq * run;
    for (int i = tid; i < total; i += threads) {
        const int x = i / run, e = i - x * run;
        dst[((q_blk + x) * dof + jb) * P + e] = value(s[i], x);
    }
}

template <int SEM>
__global__ void __launch_bounds__(kQueriesPerBlock* kMaxJointSlots)
k_stop(long long n, int dof, double t_sample, int check, PlanLimits lim, Queries in, Records out, double* __restrict__ q_stop)
{
    static_assert(!sem_matlab(SEM), "stop plans follow the C++ reference's sampler only");
    if constexpr (sem_libm(SEM)) libm::stage_tables();        // the block's LDS copy of glibc's pow tables (ltp_libm_pow.hpp)
    constexpr int kLanes = kQueriesPerBlock * kMaxJointSlots;
    __shared__ double s_rec[kLanes * 7], s_dir[kLanes], s_vd[kLanes];
    __shared__ double s_t[kMaxJointSlots][kQueriesPerBlock];
    __shared__ int s_j[kMaxJointSlots][kQueriesPerBlock];
    __shared__ int s_rej[kQueriesPerBlock], s_len[kQueriesPerBlock], s_bad[kQueriesPerBlock];

    const int x = threadIdx.x, y = threadIdx.y, JB = blockDim.y;
    const long long q_blk = (long long)blockIdx.x * kQueriesPerBlock;
    const long long q = q_blk + x;
    const bool live = q < n;
    const int nq = n - q_blk < kQueriesPerBlock ? (int)(n - q_blk) : kQueriesPerBlock;   // the block's live queries
    if (y == 0) { s_rej[x] = 0; s_len[x] = 0; s_bad[x] = 0; }
    __syncthreads();

    const bool bad_set = live && lim.set_index != nullptr && plan_set(lim, q) < 0;
    const Limits Lq = plan_limits(lim, live ? q : 0, dof);

    if (live) {
        int rej = bad_set ? 1 : 0;
        for (int j = y; j < dof; j += JB) {
            const long long ix = q * in.sq + (long long)j * in.sj;
            const double q0 = in.q_0[ix], v0 = in.v_0[ix], a0 = in.a_0[ix];
            const JointLimits L = load_limits(Lq, j);
            const bool ok = check == kStopCheckBraking ? !(dabs(a0) > L.a_max) : check_inputs_joint<SEM>(L, q0, v0, a0);
            if (!ok) rej = 1;
        }
        if (rej) atomicOr(&s_rej[x], bad_set ? 2 : 1);
    }
    __syncthreads();
    const bool rejected = (s_rej[x] & 1) != 0;
    const bool planned = s_rej[x] == 0;      // neither rejected nor a bad set index

    // cc:31-39: strict '>', first index wins, NaN never wins, init -1
    double best_t = -1.0;
    int best_j = -1;
    for (int jb = 0; jb < dof; jb += JB) {   // the same number of rounds in every wave: the staged stores contain barriers
        const int j = jb + y;
        const int nj = dof - jb < JB ? dof - jb : JB;
        if (live && j < dof) {
            const long long ix = q * in.sq + (long long)j * in.sj;
            const double q0 = in.q_0[ix], v0 = in.v_0[ix], a0 = in.a_0[ix];
            const JointLimits L = load_limits(Lq, j);
            double r[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, t[7];
            double qb = 0.0, dir = 0.0;
            MatlabCtx mc;
            opt_braking<SEM>(L.a_max, L.j_max, L.pw, t_sample, v0, a0, qb, r, dir, mc);
            cumsum7(r, t);
            if (bad_set) { zero7(t); dir = 0.0; }
            const int sl = x * nj + y;
#pragma unroll
            for (int k = 0; k < 7; ++k) s_rec[sl * 7 + k] = t[k];
            s_dir[sl] = dir;
            s_vd[sl] = L.v_max;
            if (q_stop) q_stop[ix] = planned ? q0 + qb : __builtin_nan("");   // one addition: the value cc:96 compares the goal with
            if (t[6] > best_t) { best_t = t[6]; best_j = j; }
            if (planned) {
                const int l = joint_len(t, t_sample);
                if (l < 0) atomicOr(&s_bad[x], 1);
                else atomicMax(&s_len[x], l);
            }
        }
        __syncthreads();
        store_round<7>(out.t_opt, s_rec, nq, nj, dof, q_blk, jb, [](double v, int) { return v; });
        store_round<7>(out.t_scaled, s_rec, nq, nj, dof, q_blk, jb, [&](double v, int xx) { return s_rej[xx] == 0 ? v : 0.0; });
        store_round<1>(out.dir, s_dir, nq, nj, dof, q_blk, jb, [](double v, int) { return v; });
        store_round<1>(out.v_drive, s_vd, nq, nj, dof, q_blk, jb, [](double v, int) { return v; });
        store_round<1>(out.mod, s_dir, nq, nj, dof, q_blk, jb, [](double, int) { return (signed char)0; });   // mod is 0 in every lane

        __syncthreads();   // the next round overwrites the staging arrays
    }
    s_t[y][x] = best_t;
    s_j[y][x] = best_j;
    __syncthreads();
    if (y == 0 && live) {
        double t_required = -1.0;
        int slowest = -1;
        for (int yy = 0; yy < JB; ++yy) {
            const double bt = s_t[yy][x];
            const int bj = s_j[yy][x];
            if (bj >= 0 && (bt > t_required || (bt == t_required && bj < slowest))) { t_required = bt; slowest = bj; }
        }
        int status = 0;
        if (bad_set) {
            status = kStatusBadLimitSet;
            slowest = -1;
            t_required = -1.0;
        } else {
            if (rejected) status |= kStatusInvalidInput;
            if (slowest < 0) status |= kStatusNoSlowest;      // cc:39
            if (planned && s_bad[x]) status |= kStatusNonFinite;
        }
        out.t_required[q] = t_required;
        out.slowest[q] = slowest;
        out.traj_len[q] = status == 0 ? s_len[x] : 0;
        out.status[q] = status;
    }
}

void launch_stop(hipStream_t s, long long n, int dof, double t_sample, PlanLimits lim, Queries in, Records out, double* q_stop,
                 int check, int variant)
{
    if (n <= 0 || dof <= 0) return;
    const dim3 grid((unsigned)((n + kQueriesPerBlock - 1) / kQueriesPerBlock));
    const dim3 block(kQueriesPerBlock, dof < kMaxJointSlots ? dof : kMaxJointSlots);
    if (variant & kPowLibm) hipLaunchKernelGGL(k_stop<kPowLibm>, grid, block, 0, s, n, dof, t_sample, check, lim, in, out, q_stop);
    else hipLaunchKernelGGL(k_stop<kSemCpp>, grid, block, 0, s, n, dof, t_sample, check, lim, in, out, q_stop);
}

}  // namespace ltp
