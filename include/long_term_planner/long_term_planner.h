// long_term_planner/long_term_planner.h — drop-in for the reference header of the same path.
//
// Same namespace, struct, class, constructor and method signatures as
// /root/reference/include/long_term_planner/long_term_planner.h (Trajectory :37-45, sign :54-56,
// LongTermPlanner :61-308; implementation src/long_term_planner.cc). Every method forwards to the
// MI355X library through the C ABI of include/ltp_hip.h — there is no host implementation of the
// planner arithmetic in this header or behind it, and no <Eigen/Dense> dependency (the reference
// header pulls Eigen in publicly; the root finder now lives on the device).
//
// Differences a user can observe:
//   * a HIP device is required; a missing device / HIP error throws std::runtime_error (the reference
//     has no error channel besides `bool`, and silently computing on the CPU is not offered);
//   * the reference's std::cerr diagnostic at cc:343 is not printed;
//   * corners the reference leaves undefined (out-of-range writes of the sampler,
//     non-finite switching times) are defined: dropped writes / `false`;
//   * NEW: planTrajectoryBatch(), the batched overload this library exists for; planTrajectoryBatchSharded() and
//     planEnvelopeBatchSharded(), the same over several devices from one process (contiguous query ranges, no collective).
// Threading: as with the reference, concurrent planTrajectory / planTrajectoryBatch calls on one object are allowed as
// long as no setter runs at the same time (the lazily created device handle is guarded by a mutex).
#ifndef long_term_planner_H
#define long_term_planner_H

#include <algorithm>
#include <array>
#include <cmath>
#include <cstddef>
#include <functional>
#include <math.h>
#include <mutex>
#include <numeric>
#include <stdexcept>
#include <string>
#include <vector>

#include "ltp_hip.h"

namespace long_term_planner {

/** @brief Trajectory structure (reference long_term_planner.h:37-45). q/v/a/j are [joint][sample]. */
struct Trajectory {
  int dof;
  double t_sample;
  int length;
  std::vector<std::vector<double>> q;
  std::vector<std::vector<double>> v;
  std::vector<std::vector<double>> a;
  std::vector<std::vector<double>> j;
};

/** @brief -1 / 0 / +1 (reference long_term_planner.h:54-56). */
template <typename T> int sign(T val) {
  return (T(0) < val) - (val < T(0));
}

/** @brief Result of the batched overload: switching-time records plus packed dense trajectories. */
struct BatchTrajectory {
  long long n = 0;
  int dof = 0;
  double t_sample = 0.0;
  std::vector<double> t_opt;        ///< [n][dof][7]
  std::vector<double> t_scaled;     ///< [n][dof][7]
  std::vector<double> dir;          ///< [n][dof]
  std::vector<double> v_drive;      ///< [n][dof]
  std::vector<signed char> mod;     ///< [n][dof]
  std::vector<double> t_required;   ///< [n]
  std::vector<int> slowest;         ///< [n]
  std::vector<int> length;          ///< [n] Trajectory::length, 0 if the plan failed before sampling
  std::vector<int> stored;          ///< [n] samples stored per row: length, or less when setMaxSamples() is in effect
  std::vector<int> status;          ///< [n] LTP_STATUS_* bits; planTrajectory's bool is LongTermPlanner::planOk(status)
  std::vector<unsigned long long> offsets;  ///< [n+1] plan p occupies packed[offsets[p], offsets[p+1])
  std::vector<double> packed;       ///< per plan: [q,v,a,j][joint][ltp_row_stride(length)]
  /// pointer to sample 0 of array `arr` (0=q,1=v,2=a,3=j) of joint `joint` of plan `p`
  const double* row(long long p, int arr, int joint) const {
    return packed.data() + offsets[p] + (static_cast<std::size_t>(arr) * dof + joint) * ltp_row_stride(stored[p]);
  }
  /// copy plan p out as a reference-style Trajectory
  Trajectory trajectory(long long p) const {
    Trajectory t;
    t.dof = dof; t.t_sample = t_sample; t.length = stored[p];
    std::vector<std::vector<double>>* dst[4] = {&t.q, &t.v, &t.a, &t.j};
    for (int arr = 0; arr < 4; ++arr) {
      dst[arr]->resize(dof);
      for (int i = 0; i < dof; ++i) (*dst[arr])[i].assign(row(p, arr, i), row(p, arr, i) + stored[p]);
    }
    return t;
  }
};

/** @brief Plans a trajectory for multiple joints (reference long_term_planner.h:61-308). */
class LongTermPlanner {
 private:
  int dof_;
  double t_sample_;
  std::vector<double> q_min_;
  std::vector<double> q_max_;
  std::vector<double> v_max_;
  std::vector<double> a_max_;
  std::vector<double> j_max_;

  // device-side twins of the members above; created lazily, never shared between copies. handle_ serves the
  // single-device calls, shards_[i] the i-th shard of planTrajectoryBatchSharded. mu_ guards creation/configuration:
  // the reference allows concurrent planTrajectory calls on one object (it mutates no members), so two threads'
  // first calls must not race here either.
  struct DeviceTwin {
    ltp_planner* h = nullptr;
    int device = 0;
    bool dirty = true;
  };
  mutable DeviceTwin handle_;
  mutable std::vector<DeviceTwin> shards_;
  mutable std::mutex mu_;
  int device_ = 0;
  // NEW options (defaults = the reference's behaviour); kept here so that copies and re-created handles inherit them
  int max_samples_ = 0;
  int sample_stride_ = 1;
  bool goal_check_ = false;
  int semantics_ = LTP_SEMANTICS_CPP;
  int pow_rule_ = LTP_POW_LIBM;
  int envelope_mode_ = LTP_ENVELOPE_ANALYTIC;
  // NEW limit sets (setLimitSets): [5][n_sets_ * dof_] — q_min, q_max, v_max, a_max, j_max of every set, row-major [set][joint]
  int n_sets_ = 0;
  int sets_dof_ = 0;
  std::vector<double> sets_;

  // status bits with which the reference returned before sampling: planTrajectory leaves `traj` untouched (cc:14-39)
  static constexpr int kBeforeSampling = LTP_STATUS_INVALID_INPUT | LTP_STATUS_OPT_FAILED | LTP_STATUS_NO_SLOWEST | LTP_STATUS_NONFINITE |
                                         LTP_STATUS_GOAL_OUTSIDE | LTP_STATUS_MATLAB_ERROR;

  static void raise(const ltp_planner* h, int rc, const char* what) {
    throw std::runtime_error(std::string("long_term_planner (MI355X): ") + what + " failed with code " + std::to_string(rc) +
                             (h ? std::string(": ") + ltp_last_error(h) : std::string(" (no HIP device? there is no CPU fallback)")));
  }

  void markDirty() {
    handle_.dirty = true;
    for (auto& s : shards_) s.dirty = true;
  }

  // caller holds mu_
  ltp_planner* ready(DeviceTwin& t, int device) const {
    if (t.h && t.device != device) { ltp_destroy(t.h); t.h = nullptr; }
    if (!t.h) {
      const int rc = ltp_create(0, t_sample_, nullptr, nullptr, nullptr, nullptr, nullptr, device, &t.h);
      if (rc != LTP_OK) raise(nullptr, rc, "ltp_create");
      t.device = device;
      t.dirty = true;
    }
    if (t.dirty) {
      const int n = static_cast<int>(std::min({q_min_.size(), q_max_.size(), v_max_.size(), a_max_.size(), j_max_.size()}));
      int rc = ltp_set_limits(t.h, n, q_min_.data(), q_max_.data(), v_max_.data(), a_max_.data(), j_max_.data());
      if (rc != LTP_OK) raise(t.h, rc, "ltp_set_limits");
      if ((rc = ltp_set_sample_time(t.h, t_sample_)) != LTP_OK) raise(t.h, rc, "ltp_set_sample_time");
      if ((rc = ltp_set_dof(t.h, dof_)) != LTP_OK) raise(t.h, rc, "ltp_set_dof");
      if ((rc = ltp_set_max_samples(t.h, max_samples_)) != LTP_OK) raise(t.h, rc, "ltp_set_max_samples");
      if ((rc = ltp_set_sample_stride(t.h, sample_stride_)) != LTP_OK) raise(t.h, rc, "ltp_set_sample_stride");
      if ((rc = ltp_set_goal_check(t.h, goal_check_ ? 1 : 0)) != LTP_OK) raise(t.h, rc, "ltp_set_goal_check");
      if ((rc = ltp_set_semantics(t.h, semantics_)) != LTP_OK) raise(t.h, rc, "ltp_set_semantics");
      if ((rc = ltp_set_pow_rule(t.h, pow_rule_)) != LTP_OK) raise(t.h, rc, "ltp_set_pow_rule");
      if ((rc = ltp_set_envelope_mode(t.h, envelope_mode_)) != LTP_OK) raise(t.h, rc, "ltp_set_envelope_mode");
      // (sets given for another dof are not handed over: a call that needs them then fails, as the C ABI's would)
      const int n_sets = sets_dof_ == dof_ ? n_sets_ : 0;
      const std::size_t rows = static_cast<std::size_t>(n_sets) * static_cast<std::size_t>(dof_);
      if (n_sets > 0 || ltp_get_limit_sets(t.h) > 0) {
        const double* s = sets_.data();
        rc = ltp_set_limit_sets(t.h, n_sets, s, s + rows, s + 2 * rows, s + 3 * rows, s + 4 * rows);
        if (rc != LTP_OK) raise(t.h, rc, "ltp_set_limit_sets");
      }
      t.dirty = false;
    }
    return t.h;
  }

  ltp_planner* handle() const {
    std::lock_guard<std::mutex> g(mu_);
    return ready(handle_, device_);
  }

  void release() {
    if (handle_.h) ltp_destroy(handle_.h);
    handle_.h = nullptr;
    for (auto& s : shards_)
      if (s.h) ltp_destroy(s.h);
    shards_.clear();
  }

  // sizes `out` for n queries and returns the record pointers the C ABI fills
  ltp_records prepare(long long n, BatchTrajectory& out, double& dummy_d, signed char& dummy_c) const {
    const std::size_t nd = static_cast<std::size_t>(n) * dof_;
    out.n = n; out.dof = dof_; out.t_sample = t_sample_;
    out.t_opt.assign(nd * 7, 0.0); out.t_scaled.assign(nd * 7, 0.0); out.dir.assign(nd, 0.0); out.v_drive.assign(nd, 0.0);
    out.mod.assign(nd, 0); out.t_required.assign(n, 0.0); out.slowest.assign(n, -1); out.length.assign(n, 0);
    out.status.assign(n, 0); out.offsets.assign(n + 1, 0ull); out.packed.clear(); out.stored.assign(n, 0);
    // zero-sized vectors have a null data(); the C ABI wants non-null record pointers
    return ltp_records{nd ? out.t_opt.data() : &dummy_d, nd ? out.t_scaled.data() : &dummy_d, nd ? out.dir.data() : &dummy_d,
                       nd ? out.v_drive.data() : &dummy_d, nd ? out.mod.data() : &dummy_c, out.t_required.data(),
                       out.slowest.data(), out.length.data(), out.status.data()};
  }

  long long finish(ltp_planner* h, long long n, double* packed, BatchTrajectory& out) const {
    if (packed) {
      out.packed.assign(packed, packed + out.offsets[n]);
      ltp_free_host(packed);
    }
    long long ok = 0;
    for (long long p = 0; p < n; ++p) {
      ok += planOk(out.status[p]);
      out.stored[p] = ltp_stored_samples(h, out.length[p]);
    }
    return ok;
  }

  // The frame of the planner methods (planTrajectoryBatch and its overloads, planStopBatch, the sharded call): `out` sized by
  // prepare; `call(&rec, packed)` is the method's own C call on handle h (packed: where the rows go, or null without sampling);
  // then raise with the entry's name, the rows and the count of planOk plans. A template over the call: a single planTrajectory
  // pays for this frame, which allocates nothing of its own.
  template <class Call>
  long long plannerBatch(ltp_planner* h, long long n, BatchTrajectory& out, bool sample, const char* entry, Call call) const {
    double dummy_d = 0; signed char dummy_c = 0;
    const ltp_records rec = prepare(n, out, dummy_d, dummy_c);
    double* packed = nullptr;
    const int rc = call(&rec, sample ? &packed : nullptr);
    if (rc != LTP_OK) raise(h, rc, entry);
    return finish(h, n, packed, out);
  }

  // What the *Sharded methods (`method`: the name in the texts) need first: a device list, no limit sets, and one ready handle per shard
  std::vector<ltp_planner*> shardHandles(const std::vector<int>& devices, const char* method) const {
    if (devices.empty()) throw std::runtime_error(std::string("long_term_planner (MI355X): ") + method + " needs at least one device");
    if (n_sets_ > 0) throw std::runtime_error(std::string("long_term_planner (MI355X): ") + method + " does not take limit sets (setLimitSets(0, ...) first)");
    std::vector<ltp_planner*> hs(devices.size());
    std::lock_guard<std::mutex> g(mu_);
    if (shards_.size() < devices.size()) shards_.resize(devices.size());
    for (std::size_t i = 0; i < devices.size(); ++i) hs[i] = ready(shards_[i], devices[i]);
    return hs;
  }

  // The frame of the plan*Batch reader methods (envelopes, windows, horizons, knots): the handle, `out` or a local
  // BatchTrajectory sized by prepare; `call(h, &rec, &dummy_d)` is the method's own sizing rule, dummy substitutions and C call
  // (dummy_d: a double to point at where a vector is empty); then raise with the entry's name, and the count of planOk plans.
  template <class Call>
  long long readerBatch(long long n, BatchTrajectory* out, const char* entry, Call call) {
    ltp_planner* h = handle();
    BatchTrajectory local;
    BatchTrajectory& b = out ? *out : local;
    double dummy_d = 0; signed char dummy_c = 0;
    const ltp_records rec = prepare(n, b, dummy_d, dummy_c);
    const int rc = call(h, &rec, &dummy_d);
    if (rc != LTP_OK) raise(h, rc, entry);
    long long ok = 0;
    for (long long p = 0; p < n; ++p) ok += planOk(b.status[p]);
    return ok;
  }

 public:
  /** @brief NEW: planTrajectory's bool for a batch status word: every bit but the informational LTP_STATUS_MATLAB_COMPLEX
   *  (the plan is delivered) must be clear. planTrajectory, the batch counters and bench.py all use this rule. */
  static inline bool planOk(int status) { return (status & ~LTP_STATUS_MATLAB_COMPLEX) == 0; }

  /** @brief Dummy planner (reference long_term_planner.h:103-105). */
  LongTermPlanner() : dof_(0), t_sample_(0.001) {}

  /** @brief reference long_term_planner.h:118-131 */
  LongTermPlanner(int dof, double t_sample, std::vector<double> q_min, std::vector<double> q_max, std::vector<double> v_max,
                  std::vector<double> a_max, std::vector<double> j_max)
      : dof_(dof), t_sample_(t_sample), q_min_(q_min), q_max_(q_max), v_max_(v_max), a_max_(a_max), j_max_(j_max) {}

  LongTermPlanner(const LongTermPlanner& o)
      : dof_(o.dof_), t_sample_(o.t_sample_), q_min_(o.q_min_), q_max_(o.q_max_), v_max_(o.v_max_), a_max_(o.a_max_),
        j_max_(o.j_max_), device_(o.device_), max_samples_(o.max_samples_), sample_stride_(o.sample_stride_),
        goal_check_(o.goal_check_), semantics_(o.semantics_), pow_rule_(o.pow_rule_), envelope_mode_(o.envelope_mode_),
        n_sets_(o.n_sets_), sets_dof_(o.sets_dof_), sets_(o.sets_) {}
  LongTermPlanner& operator=(const LongTermPlanner& o) {
    if (this != &o) {
      dof_ = o.dof_; t_sample_ = o.t_sample_; q_min_ = o.q_min_; q_max_ = o.q_max_; v_max_ = o.v_max_; a_max_ = o.a_max_;
      j_max_ = o.j_max_; device_ = o.device_; max_samples_ = o.max_samples_; sample_stride_ = o.sample_stride_;
      goal_check_ = o.goal_check_; semantics_ = o.semantics_; pow_rule_ = o.pow_rule_; envelope_mode_ = o.envelope_mode_;
      n_sets_ = o.n_sets_; sets_dof_ = o.sets_dof_; sets_ = o.sets_; markDirty();
    }
    return *this;
  }
  ~LongTermPlanner() { release(); }

  /** @brief reference long_term_planner.h:144-150, src/long_term_planner.cc:7-63 */
  bool planTrajectory(const std::vector<double>& q_goal, const std::vector<double>& q_0, const std::vector<double>& v_0,
                      const std::vector<double>& a_0, Trajectory& traj) {
    BatchTrajectory b;
    planTrajectoryBatch(1, q_goal.data(), q_0.data(), v_0.data(), a_0.data(), b);
    const int st = b.status[0];
    if (st & kBeforeSampling) return false;
    traj = b.trajectory(0);
    return (st & ~LTP_STATUS_MATLAB_COMPLEX) == 0;   // LTP_STATUS_END_LIMIT: false with the trajectory filled (cc:59-61)
  }

  /**
   * @brief NEW: planTrajectory with a requested duration (seconds). Every joint is time-scaled to max(duration, the slowest
   * joint's optimal time) the way cc:41-55 scales the non-slowest joints (ltp_retime_batch in ltp_hip.h); with duration at or below
   * the optimum this returns exactly what planTrajectory returns. Same return value and untouched-`traj` rules as planTrajectory.
   */
  bool planTrajectory(const std::vector<double>& q_goal, const std::vector<double>& q_0, const std::vector<double>& v_0,
                      const std::vector<double>& a_0, double duration, Trajectory& traj) {
    BatchTrajectory b;
    planTrajectoryBatchTimed(1, q_goal.data(), q_0.data(), v_0.data(), a_0.data(), &duration, b);
    const int st = b.status[0];
    if (st & kBeforeSampling) return false;
    traj = b.trajectory(0);
    return (st & ~LTP_STATUS_MATLAB_COMPLEX) == 0;
  }

  /**
   * @brief NEW: planTrajectoryBatch with a requested duration per query (`duration`: [n] seconds, or nullptr = none): plan,
   * retime (ltp_plan_retimed_host), sample. A request at or below a query's optimum leaves that query as planTrajectoryBatch plans it.
   * @return number of queries for which planTrajectory would have returned true.
   */
  long long planTrajectoryBatchTimed(long long n, const double* q_goal, const double* q_0, const double* v_0, const double* a_0,
                                     const double* duration, BatchTrajectory& out, bool sample = true) {
    ltp_planner* h = handle();
    return plannerBatch(h, n, out, sample, "ltp_plan_retimed_host", [&](const ltp_records* rec, double** packed) {
      return ltp_plan_retimed_host(h, n, q_goal, q_0, v_0, a_0, duration, 0.0, rec, out.offsets.data(), packed);
    });
  }

  /**
   * @brief NEW batched overload: n independent queries, row-major [n][dof] host arrays.
   * @return number of queries for which planTrajectory would have returned true.
   */
  long long planTrajectoryBatch(long long n, const double* q_goal, const double* q_0, const double* v_0, const double* a_0,
                                BatchTrajectory& out, bool sample = true) {
    ltp_planner* h = handle();
    return plannerBatch(h, n, out, sample, "ltp_plan_batch_host", [&](const ltp_records* rec, double** packed) {
      return ltp_plan_batch_host(h, n, q_goal, q_0, v_0, a_0, rec, out.offsets.data(), packed);
    });
  }

  /**
   * @brief NEW: stop plans (ltp_plan_stop_host): every joint of each of the n states (row-major [n][dof] host arrays) brakes to
   * rest as hard as it may, by optBraking. `out` receives the records of a planned batch (t_opt = t_scaled = the braking phases,
   * dir, v_drive = v_max, mod 0, the slowest joint, the length) and, with sample = true, the rows; `q_stop` (optional) is resized
   * to n * dof and receives the standstill positions q_0 + optBraking's q (NaN for a rejected state). check:
   * LTP_STOP_CHECK_INPUTS = checkInputs as planTrajectory applies it, LTP_STOP_CHECK_BRAKING = only |a_0| > a_max.
   * @return number of states whose stop plan is complete and ends inside the joint range (status == 0).
   */
  long long planStopBatch(long long n, const double* q_0, const double* v_0, const double* a_0, int check, BatchTrajectory& out,
                          std::vector<double>* q_stop = nullptr, bool sample = true) {
    ltp_planner* h = handle();
    return plannerBatch(h, n, out, sample, "ltp_plan_stop_host", [&](const ltp_records* rec, double** packed) {
      if (q_stop) q_stop->assign(static_cast<std::size_t>(n > 0 ? n : 0) * dof_, 0.0);
      return ltp_plan_stop_host(h, n, q_0, v_0, a_0, check, rec, q_stop && !q_stop->empty() ? q_stop->data() : nullptr,
                                out.offsets.data(), packed);
    });
  }

  /**
   * @brief NEW: limit sets — n_sets sets of joint limits for planTrajectoryBatch(..., limit_set, ...), host arrays row-major
   * [n_sets][dof] (set s, joint j at s * dof + j) for the current dof. n_sets = 0 removes them. The planner's own limits
   * (setLimits) stay what every other call uses.
   */
  bool setLimitSets(int n_sets, const double* q_min, const double* q_max, const double* v_max, const double* a_max,
                    const double* j_max) {
    if (n_sets < 0 || (n_sets > 0 && (!q_min || !q_max || !v_max || !a_max || !j_max)))
      throw std::runtime_error("long_term_planner (MI355X): setLimitSets needs n_sets >= 0 and five arrays");
    const std::size_t rows = static_cast<std::size_t>(n_sets) * static_cast<std::size_t>(dof_);
    sets_.resize(5 * rows);
    const double* src[5] = {q_min, q_max, v_max, a_max, j_max};
    for (int k = 0; k < 5; ++k)
      if (rows) std::copy(src[k], src[k] + rows, sets_.begin() + static_cast<std::ptrdiff_t>(k * rows));
    n_sets_ = n_sets;
    sets_dof_ = dof_;
    markDirty();
    return true;
  }
  /** @brief NEW: the number of limit sets (setLimitSets). */
  int limitSets() const { return n_sets_; }

  /**
   * @brief NEW: planTrajectoryBatch with per-query limit sets: query q is planned with set limit_set[q] (host [n]) of setLimitSets,
   * bit for bit what a planner whose limits are that set returns for it (ltp_plan_batch_sets_host). An index outside
   * [0, limitSets()) gives that query LTP_STATUS_BAD_LIMIT_SET and no trajectory.
   * @return number of queries for which planTrajectory would have returned true.
   */
  long long planTrajectoryBatch(long long n, const double* q_goal, const double* q_0, const double* v_0, const double* a_0,
                                const int* limit_set, BatchTrajectory& out, bool sample = true) {
    ltp_planner* h = handle();
    return plannerBatch(h, n, out, sample, "ltp_plan_batch_sets_host", [&](const ltp_records* rec, double** packed) {
      return ltp_plan_batch_sets_host(h, n, q_goal, q_0, v_0, a_0, limit_set, rec, out.offsets.data(), packed);
    });
  }

  /**
   * @brief NEW: planTrajectoryBatch over several devices from ONE process. Shard g — the contiguous
   * query range ltp_shard_range(n, g, devices.size()) — is planned on HIP device devices[g] by its own handle and host
   * thread; limits are replicated, nothing is exchanged between devices (queries are independent). `out` is
   * bit-identical to planTrajectoryBatch over all n queries. A device may be listed more than once (virtual shards).
   * @return number of queries for which planTrajectory would have returned true.
   */
  long long planTrajectoryBatchSharded(long long n, const double* q_goal, const double* q_0, const double* v_0, const double* a_0,
                                       BatchTrajectory& out, const std::vector<int>& devices, bool sample = true) {
    std::vector<ltp_planner*> hs = shardHandles(devices, "planTrajectoryBatchSharded");
    return plannerBatch(hs[0], n, out, sample, "ltp_plan_batch_multi", [&](const ltp_records* rec, double** packed) {
      return ltp_plan_batch_multi(hs.data(), static_cast<int>(hs.size()), n, q_goal, q_0, v_0, a_0, rec, out.offsets.data(), packed);
    });
  }

  /**
   * @brief NEW: plan n queries and reduce every trajectory on the device to per-joint position envelopes —
   * env[((p*dof + joint)*n_windows + w)*2 + {0,1}] = {min, max} of the q samples w*window .. (w+1)*window-1; windows past
   * the end hold the last position, plans without a trajectory NaN. The dense trajectories never exist, so this also
   * works for batches whose trajectories would not fit in memory. `out` (optional) receives the records.
   * @return number of queries for which planTrajectory would have returned true.
   */
  long long planEnvelopeBatch(long long n, const double* q_goal, const double* q_0, const double* v_0, const double* a_0,
                              int window, int n_windows, std::vector<double>& env, BatchTrajectory* out = nullptr) {
    return readerBatch(n, out, "ltp_plan_envelope_host", [&](ltp_planner* h, const ltp_records* rec, double* dummy_d) {
      const std::size_t nd = static_cast<std::size_t>(n) * dof_;
      env.assign(nd * static_cast<std::size_t>(n_windows > 0 ? n_windows : 0) * 2, 0.0);
      return ltp_plan_envelope_host(h, n, q_goal, q_0, v_0, a_0, window, n_windows, rec, env.empty() ? dummy_d : env.data());
    });
  }

  /**
   * @brief NEW: plan n queries and return, per plan, the fixed-shape horizon window of the n_samples trajectory samples
   * [k, k + n_samples), k = first_sample[p] (host [n]) or, when that is null, uniform_first (ltp_plan_window_host). `rows` is
   * resized to n * 4 * dof * R doubles, R = ltp_row_stride(n_samples): sample s of array arr (0=q,1=v,2=a,3=j) of joint i of plan
   * p at rows[((p * 4 + arr) * dof + i) * R + s]. Past the end of a plan q holds its last position and v, a, j are +0.0; plans
   * without a trajectory hold NaN; `valid` (optional) receives the number of real samples per plan. `out` (optional) receives
   * the records.
   * @return number of queries for which planTrajectory would have returned true.
   */
  long long planWindowBatch(long long n, const double* q_goal, const double* q_0, const double* v_0, const double* a_0,
                            const int* first_sample, int uniform_first, int n_samples, std::vector<double>& rows,
                            std::vector<int>* valid = nullptr, BatchTrajectory* out = nullptr) {
    return readerBatch(n, out, "ltp_plan_window_host", [&](ltp_planner* h, const ltp_records* rec, double* dummy_d) {
      rows.assign(static_cast<std::size_t>(ltp_window_elements(h, n, n_samples)), 0.0);
      if (valid) valid->assign(static_cast<std::size_t>(n > 0 ? n : 0), 0);
      return ltp_plan_window_host(h, n, q_goal, q_0, v_0, a_0, first_sample, uniform_first, n_samples, rec,
                                  rows.empty() ? dummy_d : rows.data(), valid && !valid->empty() ? valid->data() : nullptr);
    });
  }

  /**
   * @brief NEW: planWindowBatch with a stride inside the window (ltp_plan_horizon_host): element w of a row is trajectory sample
   * k + w * stride — the knots of a predictive controller's horizon, without the samples in between. `rows`, `valid` and `out`
   * as for planWindowBatch; valid counts the real elements, min(n_samples, ceil((traj_len - k) / stride)).
   * @return number of queries for which planTrajectory would have returned true.
   */
  long long planHorizonBatch(long long n, const double* q_goal, const double* q_0, const double* v_0, const double* a_0,
                             const int* first_sample, int uniform_first, int n_samples, int stride, std::vector<double>& rows,
                             std::vector<int>* valid = nullptr, BatchTrajectory* out = nullptr) {
    return readerBatch(n, out, "ltp_plan_horizon_host", [&](ltp_planner* h, const ltp_records* rec, double* dummy_d) {
      rows.assign(static_cast<std::size_t>(ltp_window_elements(h, n, n_samples)), 0.0);
      if (valid) valid->assign(static_cast<std::size_t>(n > 0 ? n : 0), 0);
      return ltp_plan_horizon_host(h, n, q_goal, q_0, v_0, a_0, first_sample, uniform_first, n_samples, stride, rec,
                                   rows.empty() ? dummy_d : rows.data(), valid && !valid->empty() ? valid->data() : nullptr);
    });
  }

  /**
   * @brief NEW: planHorizonBatch on any knot grid (ltp_plan_knots_host): element w of a row is trajectory sample k + knots[w] —
   * a horizon that is dense near the present and sparse further out, in one call. `knots`: 1 .. LTP_MAX_KNOTS non-decreasing
   * offsets in [0, 2^30] (duplicates repeat the sample, knots[0] need not be 0); any other grid throws, and nothing is launched.
   * `rows`, `valid` and `out` as for planWindowBatch with n_samples = knots.size(); valid counts the w with k + knots[w] < traj_len.
   * @return number of queries for which planTrajectory would have returned true.
   */
  long long planKnotsBatch(long long n, const double* q_goal, const double* q_0, const double* v_0, const double* a_0,
                           const int* first_sample, int uniform_first, const std::vector<int>& knots, std::vector<double>& rows,
                           std::vector<int>* valid = nullptr, BatchTrajectory* out = nullptr) {
    return readerBatch(n, out, "ltp_plan_knots_host", [&](ltp_planner* h, const ltp_records* rec, double* dummy_d) {
      const int n_knots = knots.size() > static_cast<std::size_t>(LTP_MAX_KNOTS) ? LTP_MAX_KNOTS + 1 : static_cast<int>(knots.size());
      rows.assign(static_cast<std::size_t>(ltp_window_elements(h, n, n_knots)), 0.0);
      if (valid) valid->assign(static_cast<std::size_t>(n > 0 ? n : 0), 0);
      return ltp_plan_knots_host(h, n, q_goal, q_0, v_0, a_0, first_sample, uniform_first, n_knots, knots.data(), rec,
                                 rows.empty() ? dummy_d : rows.data(), valid && !valid->empty() ? valid->data() : nullptr);
    });
  }

  /**
   * @brief NEW: plan + the stop horizons (ltp_plan_stop_knots_host): if plan p is followed up to trajectory sample k + knots[w] and
   * joint j brakes from there as hard as it may (optBraking), it comes to rest at stop[((p * 2 + 0) * dof + j) * R + w] after
   * stop[((p * 2 + 1) * dof + j) * R + w] seconds, R = ltp_row_stride(knots.size()), k = first_sample[p] (or uniform_first). `knots`:
   * the grid planKnotsBatch takes; any other grid throws, and nothing is launched. clamp_acceleration = true clamps each knot's
   * acceleration to +-a_max first; false stores NaN where |a| > a_max, per (plan, joint, knot). Past the end of a plan the robot
   * rests (its last position, 0 s); plans without a trajectory hold NaN. `valid` counts the w with k + knots[w] < traj_len.
   * @return number of queries for which planTrajectory would have returned true.
   */
  long long planStopKnotsBatch(long long n, const double* q_goal, const double* q_0, const double* v_0, const double* a_0,
                               const int* first_sample, int uniform_first, const std::vector<int>& knots, bool clamp_acceleration,
                               std::vector<double>& stop, std::vector<int>* valid = nullptr, BatchTrajectory* out = nullptr) {
    return readerBatch(n, out, "ltp_plan_stop_knots_host", [&](ltp_planner* h, const ltp_records* rec, double* dummy_d) {
      const int n_knots = knots.size() > static_cast<std::size_t>(LTP_MAX_KNOTS) ? LTP_MAX_KNOTS + 1 : static_cast<int>(knots.size());
      stop.assign(static_cast<std::size_t>(ltp_stop_knots_elements(h, n, n_knots)), 0.0);
      if (valid) valid->assign(static_cast<std::size_t>(n > 0 ? n : 0), 0);
      const int none = 0;
      return ltp_plan_stop_knots_host(h, n, q_goal, q_0, v_0, a_0, first_sample, uniform_first, n_knots,
                                      knots.empty() ? &none : knots.data(), clamp_acceleration ? LTP_STOP_ACCEL_CLAMP : LTP_STOP_ACCEL_STRICT,
                                      rec, stop.empty() ? dummy_d : stop.data(), valid && !valid->empty() ? valid->data() : nullptr);
    });
  }

  /**
   * @brief NEW: plan + the horizon envelopes (ltp_plan_envelope_knots_host): env[((p * dof + j) * M + w) * 2 + {0, 1}] = {min q, max q}
   * of joint j over the trajectory samples between the edges k + edges[w] and k + edges[w + 1], k = first_sample[p] (or
   * uniform_first), M = edges.size() - 1. `edges`: 2 .. LTP_MAX_KNOTS non-decreasing offsets in [0, 2^30], the grid planKnotsBatch
   * takes; any other grid throws, and nothing is launched. closed = false: interval w holds [k + edges[w], k + edges[w + 1]);
   * closed = true: it also holds the knot sample k + edges[w + 1]. `valid` counts the w with k + edges[w] < traj_len.
   * @return number of queries for which planTrajectory would have returned true.
   */
  long long planEnvelopeKnotsBatch(long long n, const double* q_goal, const double* q_0, const double* v_0, const double* a_0,
                                   const int* first_sample, int uniform_first, const std::vector<int>& edges, bool closed,
                                   std::vector<double>& env, std::vector<int>* valid = nullptr, BatchTrajectory* out = nullptr) {
    return readerBatch(n, out, "ltp_plan_envelope_knots_host", [&](ltp_planner* h, const ltp_records* rec, double* dummy_d) {
      const int n_intervals = edges.size() > static_cast<std::size_t>(LTP_MAX_KNOTS) ? LTP_MAX_KNOTS : static_cast<int>(edges.size()) - 1;
      env.assign(static_cast<std::size_t>(ltp_envelope_knots_elements(h, n, n_intervals)), 0.0);
      if (valid) valid->assign(static_cast<std::size_t>(n > 0 ? n : 0), 0);
      const int none = 0;
      return ltp_plan_envelope_knots_host(h, n, q_goal, q_0, v_0, a_0, first_sample, uniform_first, n_intervals,
                                          edges.empty() ? &none : edges.data(), closed ? 1 : 0, rec, env.empty() ? dummy_d : env.data(),
                                          valid && !valid->empty() ? valid->data() : nullptr);
    });
  }

  /**
   * @brief NEW: planEnvelopeKnotsBatch for any of the four arrays (ltp_plan_envelope_knots_arrays_host): `arrays` is a non-empty
   * subset of LTP_ENV_Q | LTP_ENV_V | LTP_ENV_A | LTP_ENV_J; with A selected arrays and x the rank of one among them in the order
   * q, v, a, j, env[((((p * A + x) * dof + j) * M + w) * 2 + {0, 1}] = {min, max} of that array of joint j over the interval.
   * Past the end of a plan v, a and j are 0 (an interval that reaches past the last sample also holds 0). Any other `arrays`
   * throws, and nothing is launched; everything else as planEnvelopeKnotsBatch.
   * @return number of queries for which planTrajectory would have returned true.
   */
  long long planEnvelopeKnotsArraysBatch(long long n, const double* q_goal, const double* q_0, const double* v_0, const double* a_0,
                                         const int* first_sample, int uniform_first, const std::vector<int>& edges, bool closed,
                                         int arrays, std::vector<double>& env, std::vector<int>* valid = nullptr,
                                         BatchTrajectory* out = nullptr) {
    return readerBatch(n, out, "ltp_plan_envelope_knots_arrays_host", [&](ltp_planner* h, const ltp_records* rec, double* dummy_d) {
      const int n_intervals = edges.size() > static_cast<std::size_t>(LTP_MAX_KNOTS) ? LTP_MAX_KNOTS : static_cast<int>(edges.size()) - 1;
      env.assign(static_cast<std::size_t>(ltp_envelope_knots_arrays_elements(h, n, n_intervals, arrays)), 0.0);
      if (valid) valid->assign(static_cast<std::size_t>(n > 0 ? n : 0), 0);
      const int none = 0;
      return ltp_plan_envelope_knots_arrays_host(h, n, q_goal, q_0, v_0, a_0, first_sample, uniform_first, n_intervals,
                                                 edges.empty() ? &none : edges.data(), closed ? 1 : 0, arrays, rec,
                                                 env.empty() ? dummy_d : env.data(), valid && !valid->empty() ? valid->data() : nullptr);
    });
  }

  /**
   * @brief NEW: plan + the first exits (ltp_plan_first_exit_host): exit_sample[(p * A + x) * dof + j] is the smallest trajectory
   * sample t in [k, k + horizon) at which array x of joint j of plan p lies outside its box (value < lo or value > hi; a NaN never
   * exits), LTP_EXIT_NONE for none, LTP_EXIT_NO_PLAN for a plan without a trajectory; k = first_sample[p] (or uniform_first),
   * horizon 1 .. 2^30 samples. `arrays` is a non-empty subset of LTP_ENV_Q | LTP_ENV_V | LTP_ENV_A | LTP_ENV_J, A the number of
   * selected arrays and x the rank of one among them in the order q, v, a, j. `lo` / `hi`: null, or four pointers by array (q, v, a,
   * j), each null (the plan's own limit on that side: q_min / q_max, -+v_max, -+a_max, -+j_max) or an array of dof doubles
   * (box_per_plan = false: one box per joint for the whole call) or n * dof doubles (box_per_plan = true). Sampled accelerations
   * exceed a_max by rounding in most plans: pass a margin rather than the default a box. With LTP_ENV_Q, k = 0, horizon = 2^30 and
   * no boxes, exit != LTP_EXIT_NONE is the path-limit verdict planTrajectory does not form (it checks the last position alone).
   * `first_any` (optional) receives the minimum over the table per plan. Any other `arrays` or horizon, or a box for an array that
   * is not selected, throws, and nothing is launched.
   * @return number of queries for which planTrajectory would have returned true.
   */
  long long planFirstExitBatch(long long n, const double* q_goal, const double* q_0, const double* v_0, const double* a_0,
                               const int* first_sample, int uniform_first, int horizon, int arrays, const double* const* lo,
                               const double* const* hi, bool box_per_plan, std::vector<int>& exit_sample,
                               std::vector<int>* first_any = nullptr, BatchTrajectory* out = nullptr) {
    return readerBatch(n, out, "ltp_plan_first_exit_host", [&](ltp_planner* h, const ltp_records* rec, double*) {
      exit_sample.assign(static_cast<std::size_t>(ltp_first_exit_elements(h, n, arrays)), LTP_EXIT_NONE);
      if (first_any) first_any->assign(static_cast<std::size_t>(n > 0 ? n : 0), LTP_EXIT_NONE);
      int dummy_i = 0;
      return ltp_plan_first_exit_host(h, n, q_goal, q_0, v_0, a_0, first_sample, uniform_first, horizon, arrays, lo, hi, box_per_plan ? 1 : 0,
                                      rec, exit_sample.empty() ? &dummy_i : exit_sample.data(),
                                      first_any && !first_any->empty() ? first_any->data() : nullptr);
    });
  }

  /**
   * @brief NEW: plan + settling (ltp_plan_settle_host): settle_sample[(p * A + x) * dof + j] is the trajectory sample from which
   * array x of joint j of plan p is inside its box and stays inside for the rest of [k, k + horizon) — the last outside sample + 1, k
   * where none is outside —, LTP_SETTLE_NOT_YET where sample k + horizon - 1 is outside (past the end of the plan: the resting state,
   * the last position for q and 0 for v, a, j), LTP_EXIT_NO_PLAN for a plan without a trajectory. k, horizon, `arrays`, `lo` / `hi`
   * and box_per_plan are planFirstExitBatch's. `settle_all` (optional) receives the maximum over the table per plan,
   * LTP_SETTLE_NOT_YET where any entry is. Any other `arrays` or horizon, or a box for an array that is not selected, throws, and
   * nothing is launched.
   * @return number of queries for which planTrajectory would have returned true.
   */
  long long planSettleBatch(long long n, const double* q_goal, const double* q_0, const double* v_0, const double* a_0,
                            const int* first_sample, int uniform_first, int horizon, int arrays, const double* const* lo,
                            const double* const* hi, bool box_per_plan, std::vector<int>& settle_sample,
                            std::vector<int>* settle_all = nullptr, BatchTrajectory* out = nullptr) {
    return readerBatch(n, out, "ltp_plan_settle_host", [&](ltp_planner* h, const ltp_records* rec, double*) {
      settle_sample.assign(static_cast<std::size_t>(ltp_settle_elements(h, n, arrays)), 0);
      if (settle_all) settle_all->assign(static_cast<std::size_t>(n > 0 ? n : 0), 0);
      int dummy_i = 0;
      return ltp_plan_settle_host(h, n, q_goal, q_0, v_0, a_0, first_sample, uniform_first, horizon, arrays, lo, hi, box_per_plan ? 1 : 0,
                                  rec, settle_sample.empty() ? &dummy_i : settle_sample.data(),
                                  settle_all && !settle_all->empty() ? settle_all->data() : nullptr);
    });
  }

  /**
   * @brief NEW: planEnvelopeBatch over several devices from ONE process — shard g, the contiguous query
   * range ltp_shard_range(n, g, devices.size()), is planned and reduced on HIP device devices[g] by its own handle and host
   * thread (ltp_plan_envelope_multi_host); `env` and `out` are bit-identical to planEnvelopeBatch over all n queries. This
   * is the sharded call that makes sense at scale: envelopes are 16 bytes per window, the dense rows never leave a device.
   * @return number of queries for which planTrajectory would have returned true.
   */
  long long planEnvelopeBatchSharded(long long n, const double* q_goal, const double* q_0, const double* v_0, const double* a_0,
                                     int window, int n_windows, std::vector<double>& env, const std::vector<int>& devices,
                                     BatchTrajectory* out = nullptr) {
    std::vector<ltp_planner*> hs = shardHandles(devices, "planEnvelopeBatchSharded");
    BatchTrajectory local;
    BatchTrajectory& b = out ? *out : local;
    double dummy_d = 0; signed char dummy_c = 0;
    const ltp_records rec = prepare(n, b, dummy_d, dummy_c);
    const std::size_t nd = static_cast<std::size_t>(n) * dof_;
    env.assign(nd * static_cast<std::size_t>(n_windows > 0 ? n_windows : 0) * 2, 0.0);
    const int rc = ltp_plan_envelope_multi_host(hs.data(), static_cast<int>(hs.size()), n, q_goal, q_0, v_0, a_0, window, n_windows, &rec,
                                                env.empty() ? &dummy_d : env.data());
    if (rc != LTP_OK) raise(hs[0], rc, "ltp_plan_envelope_multi_host");
    long long ok = 0;
    for (long long p = 0; p < n; ++p) ok += planOk(b.status[p]);
    return ok;
  }

  /** @brief reference long_term_planner.h:161-165, cc:68-77 */
  bool checkInputs(const std::vector<double>& q_0, const std::vector<double>& v_0, const std::vector<double>& a_0) {
    int ok = 0;
    ltp_planner* h = handle();
    const int rc = ltp_check_inputs_host(h, q_0.data(), v_0.data(), a_0.data(), &ok);
    if (rc != LTP_OK) raise(h, rc, "ltp_check_inputs_host");
    return ok != 0;
  }

  /** @brief reference long_term_planner.h:176-187 */
  inline void setLimits(std::vector<double> q_min, std::vector<double> q_max, std::vector<double> v_max,
                        std::vector<double> a_max, std::vector<double> j_max) {
    q_min_ = q_min; q_max_ = q_max; v_max_ = v_max; a_max_ = a_max; j_max_ = j_max;
    markDirty();
  }

  /** @brief reference long_term_planner.h:194-196 */
  inline void setSampleTime(double t_sample) { t_sample_ = t_sample; markDirty(); }

  /** @brief reference long_term_planner.h:203-205 (takes a double there as well) */
  inline void setDoF(double dof) { dof_ = dof; markDirty(); }

  /** @brief NEW: store only the first `max_samples` samples of each trajectory (0 = all, the reference's behaviour). */
  inline void setMaxSamples(int max_samples) {
    if (max_samples < 0) throw std::runtime_error("long_term_planner (MI355X): max_samples < 0");
    max_samples_ = max_samples; markDirty();
  }

  /** @brief NEW: store every `stride`-th sample of each trajectory (1 = every sample, the reference's behaviour). */
  inline void setSampleStride(int stride) {
    if (stride < 1) throw std::runtime_error("long_term_planner (MI355X): stride < 1");
    sample_stride_ = stride; markDirty();
  }

  /** @brief NEW, off by default: reject a q_goal outside [q_min, q_max] before planning (LTP_STATUS_GOAL_OUTSIDE;
   * planTrajectory then returns false with traj untouched). The reference leaves q_goal unchecked (cc:68-77). */
  inline void setGoalCheck(bool enabled) { goal_check_ = enabled; markDirty(); }

  /** @brief NEW, default false: follow the MATLAB original LTPlanner.m where the C++ translation diverges
   * from it (positional root picks, zeros instead of failures, no position limits, 1-based sampler; ltp_hip.h
   * LTP_SEMANTICS_MATLAB). BatchTrajectory::status may then carry LTP_STATUS_MATLAB_ERROR / LTP_STATUS_MATLAB_COMPLEX. */
  inline void setMatlabSemantics(bool enabled) { semantics_ = enabled ? LTP_SEMANTICS_MATLAB : LTP_SEMANTICS_CPP; markDirty(); }

  /** @brief NEW, default TRUE: the reference's pow(x, 3 | 4 | 6) and pow(x, 1.0 / 2) calls (cc:125-331, 378-621) are formed as glibc's
   * pow forms them, operation for operation: every switching time and every sample has the bits of the reference built with gcc +
   * glibc (>= 2.28) on a host with FMA (ltp_hip.h LTP_POW_LIBM). false: the correctly rounded powers instead (LTP_POW_EXACT: within
   * 1 ulp of any libm, switching times within 5e-11 s of the above). powRuleMatchingHostLibm() tells which one this host's libm is. */
  inline void setLibmPow(bool enabled) { pow_rule_ = enabled ? LTP_POW_LIBM : LTP_POW_EXACT; markDirty(); }

  /** @brief NEW: which pow rule reproduces the libm of THIS process (the one a reference built on this host calls): LTP_POW_LIBM
   * (the default rule gives that reference's records bit for bit), LTP_POW_EXACT (setLibmPow(false) does), or -1 — a third libm:
   * about one power in a thousand differs in its last bit from either rule, i.e. ~2 plans per million carry a jerk sample beyond
   * 1e-9 of that reference whichever rule is set. Host only, ~20 ms, no GPU work (ltp_hip.h ltp_host_libm_pow_rule). */
  static inline int powRuleMatchingHostLibm() { return ltp_host_libm_pow_rule(0, nullptr, nullptr); }

  /** @brief NEW, default TRUE since round 6: the envelope calls evaluate only the samples at the ends of each run
   * stretch and either side of the real roots of q'(m) instead of every sample (ltp_hip.h LTP_ENVELOPE_ANALYTIC): identical to the
   * exhaustive result in 8.8e9 soaked window values, <= 1e-12 by construction. false: every sample (the rows' bits by construction). */
  inline void setAnalyticEnvelopes(bool enabled) { envelope_mode_ = enabled ? LTP_ENVELOPE_ANALYTIC : LTP_ENVELOPE_EXHAUSTIVE; markDirty(); }

  /** @brief NEW: HIP device ordinal used by this planner (default 0). */
  inline void setDevice(int device) { if (device != device_) { device_ = device; markDirty(); } }

  /** @brief NEW: the C-ABI handle, for callers that drive the device-pointer entry points of ltp_hip.h directly. */
  ltp_planner* nativeHandle() { return handle(); }

 protected:
  /** @brief reference long_term_planner.h:223-231, cc:82-353 */
  bool optSwitchTimes(int joint, double q_goal, double q_0, double v_0, double a_0, double v_drive, std::array<double, 7>& t,
                      double& dir, char& mod_jerk_profile) {
    int ok = 0;
    ltp_planner* h = handle();
    const int rc = ltp_opt_switch_times_host(h, joint, q_goal, q_0, v_0, a_0, v_drive, t.data(), &dir, &mod_jerk_profile, &ok);
    if (rc != LTP_OK) raise(h, rc, "ltp_opt_switch_times_host");
    return ok != 0;
  }

  /** @brief reference long_term_planner.h:249-259, cc:358-645 */
  bool timeScaling(int joint, double q_goal, double q_0, double v_0, double a_0, double dir, double t_required,
                   std::array<double, 7>& scaled_t, double& v_drive, char& mod_jerk_profile) {
    int ok = 0;
    ltp_planner* h = handle();
    const int rc = ltp_time_scaling_host(h, joint, q_goal, q_0, v_0, a_0, dir, t_required, scaled_t.data(), &v_drive,
                                         &mod_jerk_profile, &ok, nullptr);
    if (rc != LTP_OK) raise(h, rc, "ltp_time_scaling_host");
    return ok != 0;
  }

  /** @brief reference long_term_planner.h:279-285, cc:650-701 (writes t_rel[0..2] only) */
  bool optBraking(int joint, double v_0, double a_0, double& q, std::array<double, 7>& t_rel, double& dir) {
    ltp_planner* h = handle();
    const int rc = ltp_opt_braking_host(h, joint, v_0, a_0, &q, t_rel.data(), &dir);
    if (rc != LTP_OK) raise(h, rc, "ltp_opt_braking_host");
    return true;
  }

  /** @brief reference long_term_planner.h:299-307, cc:706-841 */
  Trajectory getTrajectory(const std::vector<std::array<double, 7>>& t, const std::vector<double>& dir,
                           const std::vector<char>& mod_jerk_profile, const std::vector<double>& q_0,
                           const std::vector<double>& v_0, const std::vector<double>& a_0, const std::vector<double>& v_drive) {
    ltp_planner* h = handle();
    BatchTrajectory b;
    b.n = 1; b.dof = dof_; b.t_sample = t_sample_;
    b.length.assign(1, 0); b.status.assign(1, 0); b.offsets.assign(2, 0ull); b.stored.assign(1, 0);
    std::vector<signed char> mod(mod_jerk_profile.begin(), mod_jerk_profile.end());
    double* packed = nullptr;
    const int rc = ltp_get_trajectory_host(h, 1, t.empty() ? nullptr : t[0].data(), dir.data(), mod.data(), q_0.data(), v_0.data(),
                                           a_0.data(), v_drive.data(), b.length.data(), b.status.data(), b.offsets.data(), &packed);
    if (rc != LTP_OK) raise(h, rc, "ltp_get_trajectory_host");
    if (packed) {
      b.packed.assign(packed, packed + b.offsets[1]);
      ltp_free_host(packed);
    }
    b.stored[0] = ltp_stored_samples(h, b.length[0]);
    return b.trajectory(0);
  }
};
}  // namespace long_term_planner

#endif  // long_term_planner_H
