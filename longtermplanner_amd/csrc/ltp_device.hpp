// ltp_device.hpp — small device-side helpers shared by the kernel translation units.
#pragma once
#include "ltp_kernels.hpp"
#include "ltp_profile.hpp"

namespace ltp {

typedef double double2_t __attribute__((ext_vector_type(2)));
typedef float float4_t __attribute__((ext_vector_type(4)));

// 16-byte store unit of an output row: 2 doubles or 4 floats
template <typename T> struct OutVec;
template <> struct OutVec<double> { typedef double2_t type; static constexpr int N = 2; };
template <> struct OutVec<float> { typedef float4_t type; static constexpr int N = 4; };

LTP_DEV LimPow load_limit_powers(const Limits& lim, int j)
{
    const double* w = lim.pw + (long long)j * kLimPowN;
    return LimPow{w[0], w[1], w[2], w[3], w[4], w[5], w[6]};
}

LTP_DEV JointLimits load_limits(const Limits& lim, int j)
{
    JointLimits L;
    L.q_min = lim.q_min[j];
    L.q_max = lim.q_max[j];
    L.v_max = lim.v_max[j];
    L.a_max = lim.a_max[j];
    L.j_max = lim.j_max[j];
    L.pw = load_limit_powers(lim, j);
    return L;
}

// The set plan p reads (ltp_bind_limit_sets): set_index[p], or -1 when it lies outside [0, n_sets) (LTP_STATUS_BAD_LIMIT_SET)
LTP_DEV int plan_set(const PlanLimits& lim, long long p)
{
    const int s = lim.set_index[p];
    return s >= 0 && s < lim.n_sets ? s : -1;
}

// The one place that decides where plan p reads its limits: the handle's own without a bound index, else its set of the set table.
// A bad index reads set 0 (never outside the table); the plan is then failed by the stage kernels, so no consumer uses what it reads.
LTP_DEV Limits plan_limits(const PlanLimits& lim, long long p, int dof)
{
    if (!lim.set_index) return lim;
    const int s = plan_set(lim, p);
    const long long o = (long long)(s < 0 ? 0 : s) * dof, rows = lim.set_rows;
    return Limits{lim.sets + o, lim.sets + rows + o, lim.sets + 2 * rows + o, lim.sets + 3 * rows + o, lim.sets + 4 * rows + o,
                  lim.set_pw + o * kLimPowN};
}

// Lane idx = local * dof + j of a lane-per-(plan, joint) kernel (launch_lanes, ltp_kernels.hpp) is joint j of plan p = first + local;
// the lanes behind the range's last pair are not live. start(): the state "before sample 0" (cc:810-812), loaded on request.
struct PlanLane {
    bool live;
    long long local, p;
    int j;
    LTP_DEV void start(const Queries& in, double& q, double& v, double& a) const
    {
        const long long ix = p * in.sq + (long long)j * in.sj;
        q = in.q_0[ix];
        v = in.v_0[ix];
        a = in.a_0[ix];
    }
};
LTP_DEV PlanLane plan_lane(const PlanRange& r)
{
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long local = idx / r.dof;
    return PlanLane{idx < r.count * r.dof, local, r.first + local, (int)(idx - local * r.dof)};
}

// planTrajectory's end-limit verdict (cc:59-61): q, the last position of a joint's trajectory, lies outside the joint's range
LTP_DEV bool beyond_end_limits(double q, double q_min, double q_max) { return q < q_min || q > q_max; }

// (int)ceil(t[6]/Ts) + 1 of one joint (cc:718), or -1 if any of its switching times is not finite or the length does
// not fit an int (both DEFINED here: the reference converts out-of-range doubles to int, which is undefined)
LTP_DEV int joint_len(const double (&t)[7], double t_sample)
{
    bool finite = true;
#pragma unroll
    for (int k = 0; k < 7; ++k) finite = finite && dfinite(t[k]);
    const double len = dceil(t[6] / t_sample) + 1.0;
    return (finite && len < 2147483647.0) ? (int)len : -1;
}

// Samples stored per row: every rows.stride-th sample (0, stride, 2*stride, ...), at most rows.max_samples of them.
// {0, 1} stores whole trajectories, which is the reference's behaviour.
LTP_HD int stored_len(int len, RowSpec rows)
{
    if (len <= 0) return 0;
    const int st = rows.stride > 1 ? rows.stride : 1;
    const int cnt = (len + st - 1) / st;
    return (rows.max_samples > 0 && cnt > rows.max_samples) ? rows.max_samples : cnt;
}

// (a plan's size in the tile and the fit rule: plan_size, plan_beyond_tile, ltp_sampler_policy.hpp)

// 64-bit values between lanes, as two 32-bit moves. uniform64: a value every lane holds alike -> scalar registers.
template <class Move32> LTP_DEV unsigned long long lane_move64(unsigned long long x, Move32 move)
{
    return ((unsigned long long)(unsigned)move((int)(unsigned)(x >> 32)) << 32) | (unsigned long long)(unsigned)move((int)(unsigned)x);
}
LTP_DEV unsigned long long uniform64(unsigned long long x) { return lane_move64(x, [](int w) { return __builtin_amdgcn_readfirstlane(w); }); }
LTP_DEV unsigned long long readlane64(unsigned long long x, int lane) { return lane_move64(x, [=](int w) { return __builtin_amdgcn_readlane(w, lane); }); }
LTP_DEV unsigned long long shfl64(unsigned long long x, int lane) { return lane_move64(x, [=](int w) { return __shfl(w, lane); }); }

}  // namespace ltp
