// stop_dropin_test.cc — LongTermPlanner::planStopBatch through the drop-in header, against two lanes computed by hand.
// Compiled by tests/test_gpu_stop.py with plain g++ against include/ and libltp_hip.so; needs the GPU. argv[1] is not read;
// argv[2] receives q_stop (2 doubles), the slowest joint's time (1 double) and the length (as a double).
//
// One state of two joints, limits v 1 / a 2 / j 16, sample time 2^-7 s (every quantity below is exact in binary64 but the cubes):
//   joint 0 at rest (v = a = 0): optBraking takes the square-root branch with all three phases 0: t = 0, dir = 0, q_stop = q_0.
//   joint 1 with v = 0.75, a = 0: dir = -1; t_rel = {(2 - 0) / 16, 0.75 / 2 - (0.125 + 0.125) / 2, 2 / 16} = {0.125, 0.25, 0.125};
//     q = -0.75 * 0.5 + 16 * (0.125^2 * 0.375 / 2 + 0.125 * 0.125^2 / 2) + 2 * (0.25^2 / 2 + 0.25 * 0.125) = -0.1875 (the two cubes
//     cancel), so the joint comes to rest 0.1875 rad further on after 0.5 s = 64 samples: length 65, slowest joint 1.
#include <cmath>
#include <cstdio>
#include <vector>

#include "long_term_planner/long_term_planner.h"

#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); return 1; } \
  } while (0)

int main(int argc, char** argv) {
  using long_term_planner::BatchTrajectory;
  using long_term_planner::LongTermPlanner;
  const double ts = 0.0078125;
  LongTermPlanner ltp(2, ts, {-3.0, -3.0}, {3.0, 3.0}, {1.0, 1.0}, {2.0, 2.0}, {16.0, 16.0});
  const double q_0[2] = {0.5, -1.0}, v_0[2] = {0.0, 0.75}, a_0[2] = {0.0, 0.0};
  BatchTrajectory out;
  std::vector<double> q_stop;
  const long long ok = ltp.planStopBatch(1, q_0, v_0, a_0, LTP_STOP_CHECK_INPUTS, out, &q_stop, true);
  CHECK(ok == 1 && out.status[0] == 0);
  CHECK(q_stop.size() == 2 && q_stop[0] == 0.5 && std::fabs(q_stop[1] - (-1.0 + 0.1875)) <= 1e-12);
  const double t1[7] = {0.125, 0.375, 0.5, 0.5, 0.5, 0.5, 0.5};
  for (int k = 0; k < 7; ++k) {
    CHECK(out.t_opt[k] == 0.0 && out.t_scaled[k] == 0.0);
    CHECK(out.t_opt[7 + k] == t1[k] && out.t_scaled[7 + k] == t1[k]);
  }
  CHECK(out.dir[0] == 0.0 && out.dir[1] == -1.0 && out.mod[0] == 0 && out.mod[1] == 0);
  CHECK(out.v_drive[0] == 1.0 && out.v_drive[1] == 1.0);
  CHECK(out.slowest[0] == 1 && out.t_required[0] == 0.5 && out.length[0] == 65 && out.stored[0] == 65);
  // the rows: joint 0 rests at q_0 throughout; joint 1 ends next to q_stop. The row end is getTrajectory's, whose jerk samples are
  // placed on the sample grid (cc:735-807), q_stop the closed form: at this coarse sample time they differ by a few 1e-3 rad and
  // the last velocity is within two samples of full deceleration (2 * a_max * t_sample) of rest.
  for (int s = 0; s < 65; ++s) CHECK(out.row(0, 0, 0)[s] == 0.5 && out.row(0, 1, 0)[s] == 0.0);
  CHECK(std::fabs(out.row(0, 0, 1)[64] - q_stop[1]) <= 1e-2 && std::fabs(out.row(0, 1, 1)[64]) <= 2.0 * 2.0 * ts);
  // a state whose acceleration is beyond a_max is rejected in both modes, and its q_stop is NaN
  const double a_bad[2] = {0.0, 2.5};
  for (int check : {LTP_STOP_CHECK_INPUTS, LTP_STOP_CHECK_BRAKING}) {
    BatchTrajectory rej;
    std::vector<double> qs;
    CHECK(ltp.planStopBatch(1, q_0, v_0, a_bad, check, rej, &qs, false) == 0);
    CHECK(rej.status[0] == LTP_STATUS_INVALID_INPUT && rej.length[0] == 0 && std::isnan(qs[0]) && std::isnan(qs[1]));
  }
  // a default-constructed planner has dof 0: every state fails with no slowest joint (cc:39), as planTrajectoryBatch reports it
  for (bool sample : {false, true}) {
    LongTermPlanner none;
    BatchTrajectory b;
    std::vector<double> qs;
    CHECK(none.planStopBatch(1, q_0, v_0, a_0, LTP_STOP_CHECK_INPUTS, b, &qs, sample) == 0);
    CHECK(b.status[0] == LTP_STATUS_NO_SLOWEST && b.slowest[0] == -1 && b.length[0] == 0);
    CHECK(b.offsets.size() == 2 && b.offsets[0] == 0 && b.offsets[1] == 0 && b.packed.empty());
  }
  if (argc > 2) {
    std::FILE* f = std::fopen(argv[2], "wb");
    CHECK(f != nullptr);
    const double w[4] = {q_stop[0], q_stop[1], out.t_required[0], static_cast<double>(out.length[0])};
    CHECK(std::fwrite(w, sizeof(double), 4, f) == 4);
    std::fclose(f);
  }
  std::printf("stop_dropin_test: ok\n");
  return 0;
}
