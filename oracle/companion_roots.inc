/*
 * oracle/companion_roots.inc — TEST INFRASTRUCTURE ONLY (see ltp_oracle.c header).
 *
 * Type-generic body (REAL = double or float, FN(x) = name mangler) of the
 * polynomial root finder the reference delegates to a third-party library:
 *
 *   reference include/long_term_planner/roots.h:22-34  roots<T>()
 *       builds the monic companion matrix and calls
 *       Eigen::EigenSolver<Matrix<T,Dynamic,Dynamic>>(C).eigenvalues()
 *   reference include/long_term_planner/roots.h:43-50  getSmallestPositiveNonComplexRoot<T>()
 *
 * Eigen (pinned "3.4" by the reference's CMakeLists.txt:8 / README.md:39-43)
 * is NOT vendored under /root/reference and is not installed in this image,
 * so this file restates Eigen 3.4's published algorithm for that call:
 *   EigenSolver::compute  ->  RealSchur::compute
 *     (scale by max|a_ij|, Householder Hessenberg reduction, then the
 *      EISPACK-hqr2 / JAMA-derived Francis double-shift QR with Wilkinson's
 *      ad-hoc shift at iteration 10 and MATLAB's at iteration 30,
 *      40*n total iterations), then eigenvalues read off the quasi-triangular
 *      T: 1x1 blocks are real (imag == 0 exactly), 2x2 blocks that
 *      splitOffTwoRows could not split are complex pairs (+im first).
 * For a companion matrix the Hessenberg reduction is the identity (the tail
 * below every sub-diagonal entry is exactly zero, so every Householder
 * reflector has tau == 0), which is why it does not appear below.
 *
 * Behaviour the reference leaves undefined and this oracle DEFINES
 * (SURVEY.md App. D-3): a non-finite matrix or a non-converged iteration
 * (Eigen leaves the eigenvalue vector uninitialised) yields NaN eigenvalues,
 * i.e. no admissible root.
 */

#define RS_MAXN 8

static REAL FN(rs_abs)(REAL x) { return x < 0 ? -x : x; }
static REAL FN(rs_max)(REAL a, REAL b) { return a < b ? b : a; }

/* Eigen MatrixBase::makeHouseholder for a 3- or 2-vector (c0, tail...) */
static void FN(rs_householder)(REAL c0, const REAL *tail, int ntail, REAL *ess, REAL *tau, REAL *beta)
{
    REAL tail_sq = 0;
    int i;
    if (ntail == 2) tail_sq = tail[0] * tail[0] + tail[1] * tail[1];
    else if (ntail == 1) tail_sq = tail[0] * tail[0];
    if (tail_sq <= REAL_MIN) {
        ltpo_schur_flags |= (ntail == 2) ? LTPO_F_HH3_SMALL_TAIL : LTPO_F_HH2_SMALL_TAIL;
        *tau = 0;
        *beta = c0;
        for (i = 0; i < ntail; i++) ess[i] = 0;
    } else {
        REAL b = REAL_SQRT(c0 * c0 + tail_sq);
        if (c0 >= 0) b = -b;
        for (i = 0; i < ntail; i++) ess[i] = tail[i] / (c0 - b);
        *tau = (b - c0) / b;
        *beta = b;
    }
}

/* Eigen JacobiRotation::makeGivens (real scalars) */
static void FN(rs_givens)(REAL p, REAL q, REAL *c, REAL *s)
{
    if (q == 0) {
        ltpo_schur_flags |= LTPO_F_GIVENS_Q0;
        *c = p < 0 ? (REAL)-1 : (REAL)1;
        *s = 0;
    } else if (p == 0) {
        ltpo_schur_flags |= LTPO_F_GIVENS_P0;
        *c = 0;
        *s = q < 0 ? (REAL)1 : (REAL)-1;
    } else if (FN(rs_abs)(p) > FN(rs_abs)(q)) {
        REAL t = q / p;
        ltpo_schur_flags |= LTPO_F_GIVENS_P_LARGER;
        REAL u = REAL_SQRT((REAL)1 + t * t);
        if (p < 0) u = -u;
        *c = (REAL)1 / u;
        *s = -t * *c;
    } else {
        REAL t = p / q;
        ltpo_schur_flags |= LTPO_F_GIVENS_Q_LARGER;
        REAL u = REAL_SQRT((REAL)1 + t * t);
        if (q < 0) u = -u;
        *s = -(REAL)1 / u;
        *c = -t * *s;
    }
}

/*
 * Eigenvalues of the companion matrix of p[0..n] (highest coefficient first).
 * re/im receive n values in Eigen's output order. Returns 0 on success,
 * 1 = no convergence, 2 = non-finite input (re/im are NaN-filled then).
 */
static int FN(companion_eigenvalues)(const REAL *p, int n, REAL *re, REAL *im)
{
    REAL T[RS_MAXN][RS_MAXN];
    REAL scale = 0, norm = 0, exshift = 0, consider_zero;
    int i, j, k, iu, iter = 0, total_iter = 0, max_iters = 40 * n;
    const REAL nanv = (REAL)NAN;

    /* diagnostics of this solve (ltpo_last_schur_*): none of them feeds the arithmetic */
    ltpo_schur_flags = 0;
    ltpo_schur_iterations = 0;
    { int w_; for (w_ = 0; w_ < 9; w_++) ltpo_schur_window_steps[w_] = 0; for (w_ = 0; w_ < 81; w_++) ltpo_schur_iliu_steps[w_] = 0; }
    for (i = 0; i < n; i++) { re[i] = nanv; im[i] = nanv; }
    if (n < 1 || n > RS_MAXN) return 2;

    /* roots.h:26-31: C = 0; sub-diagonal ones; last column (-1*p[n-i])/p[0] */
    for (i = 0; i < n; i++) for (j = 0; j < n; j++) T[i][j] = 0;
    for (i = 1; i < n; i++) T[i][i - 1] = 1;
    for (i = 0; i < n; i++) T[i][n - 1] = ((REAL)-1 * p[n - i]) / p[0];
    for (i = 0; i < n; i++) {
        REAL c = T[i][n - 1];
        if (!(c - c == 0)) { ltpo_schur_flags |= LTPO_F_NONFINITE_MATRIX; return 2; } /* inf or NaN */
    }

    /* RealSchur::compute: scale so that max|a_ij| == 1 */
    for (i = 0; i < n; i++) for (j = 0; j < n; j++) scale = FN(rs_max)(scale, FN(rs_abs)(T[i][j]));
    if (scale < REAL_MIN) { /* matrix considered zero: T = 0 */
        ltpo_schur_flags |= LTPO_F_CONSIDERED_ZERO;
        for (i = 0; i < n; i++) { re[i] = 0; im[i] = 0; }
        return 0;
    }
    for (i = 0; i < n; i++) for (j = 0; j < n; j++) T[i][j] = T[i][j] / scale;

    /* computeNormOfT: upper Hessenberg 1-norm-like sum */
    for (j = 0; j < n; j++) {
        int lim = (n < j + 2) ? n : j + 2;
        REAL colsum = 0;
        for (i = 0; i < lim; i++) colsum += FN(rs_abs)(T[i][j]);
        norm += colsum;
    }
    consider_zero = FN(rs_max)(norm * (REAL_EPS * REAL_EPS), REAL_MIN);

    iu = n - 1;
    if (norm != 0) {
        while (iu >= 0) {
            /* findSmallSubdiagEntry */
            int il = iu;
            while (il > 0) {
                REAL s = FN(rs_abs)(T[il - 1][il - 1]) + FN(rs_abs)(T[il][il]);
                s = FN(rs_max)(s * REAL_EPS, consider_zero);
                if (FN(rs_abs)(T[il][il - 1]) <= s) break;
                il--;
            }
            if (il == iu) { /* one root found */
                ltpo_schur_flags |= LTPO_F_DEFLATE_ONE;
                T[iu][iu] = T[iu][iu] + exshift;
                if (iu > 0) T[iu][iu - 1] = 0;
                iu--;
                iter = 0;
            } else if (il == iu - 1) { /* two roots found: splitOffTwoRows */
                REAL pp = (REAL)0.5 * (T[iu - 1][iu - 1] - T[iu][iu]);
                REAL qq = pp * pp + T[iu][iu - 1] * T[iu - 1][iu];
                T[iu][iu] += exshift;
                T[iu - 1][iu - 1] += exshift;
                if (qq >= 0) { /* two real eigenvalues: rotate to triangular */
                    REAL z = REAL_SQRT(FN(rs_abs)(qq));
                    REAL c, s;
                    ltpo_schur_flags |= (pp >= 0) ? LTPO_F_DEFLATE_TWO_REAL_P_NONNEG : LTPO_F_DEFLATE_TWO_REAL_P_NEG;
                    if (pp >= 0) FN(rs_givens)(pp + z, T[iu][iu - 1], &c, &s);
                    else FN(rs_givens)(pp - z, T[iu][iu - 1], &c, &s);
                    /* rightCols(n-iu+1).applyOnTheLeft(iu-1, iu, rot.adjoint()) */
                    for (k = iu - 1; k < n; k++) {
                        REAL x = T[iu - 1][k], y = T[iu][k];
                        T[iu - 1][k] = c * x + (-s) * y;
                        T[iu][k] = s * x + c * y;
                    }
                    /* topRows(iu+1).applyOnTheRight(iu-1, iu, rot) */
                    for (k = 0; k <= iu; k++) {
                        REAL x = T[k][iu - 1], y = T[k][iu];
                        T[k][iu - 1] = c * x + (-s) * y;
                        T[k][iu] = s * x + c * y;
                    }
                    T[iu][iu - 1] = 0;
                } else {
                    ltpo_schur_flags |= LTPO_F_DEFLATE_TWO_COMPLEX;
                }
                if (iu > 1) T[iu - 1][iu - 2] = 0;
                iu -= 2;
                iter = 0;
            } else { /* no convergence yet: one Francis double-shift step */
                REAL sh0, sh1, sh2, v[3] = {0, 0, 0}, ess[2], tau, beta;
                int im_;
                /* computeShift */
                sh0 = T[iu][iu];
                sh1 = T[iu - 1][iu - 1];
                sh2 = T[iu][iu - 1] * T[iu - 1][iu];
                if (iter == 10) { /* Wilkinson's original ad hoc shift */
                    REAL s;
                    ltpo_schur_flags |= (il == 0 && iu == 3) ? LTPO_F_SHIFT10_WINDOW03 : LTPO_F_SHIFT10_OTHER;
                    exshift += sh0;
                    for (i = 0; i <= iu; i++) T[i][i] -= sh0;
                    s = FN(rs_abs)(T[iu][iu - 1]) + FN(rs_abs)(T[iu - 1][iu - 2]);
                    sh0 = (REAL)0.75 * s;
                    sh1 = (REAL)0.75 * s;
                    sh2 = (REAL)-0.4375 * s * s;
                }
                if (iter == 30) { /* MATLAB's new ad hoc shift */
                    REAL s = (sh1 - sh0) / (REAL)2.0;
                    s = s * s + sh2;
                    ltpo_schur_flags |= (s > 0) ? LTPO_F_SHIFT30_POSITIVE : LTPO_F_SHIFT30_NOT_POSITIVE;
                    if (il == 0 && iu == 3) ltpo_schur_flags |= LTPO_F_ITER30_WINDOW03;
                    if (s == 0) ltpo_schur_flags |= LTPO_F_SHIFT30_ZERO;
                    if (s > 0) {
                        s = REAL_SQRT(s);
                        if (sh1 < sh0) s = -s;
                        s = s + (sh1 - sh0) / (REAL)2.0;
                        s = sh0 - sh2 / s;
                        exshift += s;
                        for (i = 0; i <= iu; i++) T[i][i] -= s;
                        sh0 = sh1 = sh2 = (REAL)0.964;
                    }
                }
                iter = iter + 1;
                total_iter = total_iter + 1;
                ltpo_schur_iliu_steps[il * 9 + iu]++;
                ltpo_schur_window_steps[iu - il + 1 <= 8 ? iu - il + 1 : 8]++;
                if (total_iter > max_iters) break;
                if (il == 0 && iu == 3) ltpo_schur_flags |= LTPO_F_STEP_WINDOW03;
                else if (n >= 5) ltpo_schur_flags |= LTPO_F_STEP_OTHER_N5;
                /* initFrancisQRStep */
                for (im_ = iu - 2; im_ >= il; --im_) {
                    REAL Tmm = T[im_][im_];
                    REAL r = sh0 - Tmm;
                    REAL s = sh1 - Tmm;
                    REAL lhs, rhs;
                    v[0] = (r * s - sh2) / T[im_ + 1][im_] + T[im_][im_ + 1];
                    v[1] = T[im_ + 1][im_ + 1] - Tmm - r - s;
                    v[2] = T[im_ + 2][im_ + 1];
                    if (im_ == il) break;
                    lhs = T[im_][im_ - 1] * (FN(rs_abs)(v[1]) + FN(rs_abs)(v[2]));
                    rhs = v[0] * (FN(rs_abs)(T[im_ - 1][im_ - 1]) + FN(rs_abs)(Tmm) + FN(rs_abs)(T[im_ + 1][im_ + 1]));
                    if (FN(rs_abs)(lhs) < REAL_EPS * rhs) break;
                }
                if (im_ > il) ltpo_schur_flags |= LTPO_F_START_BELOW_TOP;
                /* performFrancisQRStep */
                for (k = im_; k <= iu - 2; ++k) {
                    int first = (k == im_);
                    REAL w[3];
                    if (first) { w[0] = v[0]; w[1] = v[1]; w[2] = v[2]; }
                    else { w[0] = T[k][k - 1]; w[1] = T[k + 1][k - 1]; w[2] = T[k + 2][k - 1]; }
                    FN(rs_householder)(w[0], &w[1], 2, ess, &tau, &beta);
                    if (beta == 0) ltpo_schur_flags |= LTPO_F_BETA_ZERO;
                    if (beta != 0) {
                        int rmax = (iu < k + 3) ? iu : k + 3;
                        if (first && k > il) T[k][k - 1] = -T[k][k - 1];
                        else if (!first) T[k][k - 1] = beta;
                        if (tau != 0) {
                            /* block(k,k,3,n-k).applyHouseholderOnTheLeft */
                            for (j = k; j < n; j++) {
                                REAL tmp = ess[0] * T[k + 1][j] + ess[1] * T[k + 2][j];
                                tmp += T[k][j];
                                T[k][j] -= tau * tmp;
                                T[k + 1][j] -= (tau * ess[0]) * tmp;
                                T[k + 2][j] -= (tau * ess[1]) * tmp;
                            }
                            /* block(0,k,min(iu,k+3)+1,3).applyHouseholderOnTheRight */
                            for (i = 0; i <= rmax; i++) {
                                REAL tmp = T[i][k + 1] * ess[0] + T[i][k + 2] * ess[1];
                                tmp += T[i][k];
                                T[i][k] -= tau * tmp;
                                T[i][k + 1] -= (tau * tmp) * ess[0];
                                T[i][k + 2] -= (tau * tmp) * ess[1];
                            }
                        }
                    }
                }
                {
                    REAL w0 = T[iu - 1][iu - 2], w1 = T[iu][iu - 2];
                    FN(rs_householder)(w0, &w1, 1, ess, &tau, &beta);
                    if (beta == 0) ltpo_schur_flags |= LTPO_F_BETA_ZERO;
                    if (beta != 0) {
                        T[iu - 1][iu - 2] = beta;
                        if (tau != 0) {
                            for (j = iu - 1; j < n; j++) {
                                REAL tmp = ess[0] * T[iu][j];
                                tmp += T[iu - 1][j];
                                T[iu - 1][j] -= tau * tmp;
                                T[iu][j] -= (tau * ess[0]) * tmp;
                            }
                            for (i = 0; i <= iu; i++) {
                                REAL tmp = T[i][iu] * ess[0];
                                tmp += T[i][iu - 1];
                                T[i][iu - 1] -= tau * tmp;
                                T[i][iu] -= (tau * tmp) * ess[0];
                            }
                        }
                    }
                }
                /* clean up pollution due to round-off errors */
                for (i = im_ + 2; i <= iu; ++i) {
                    T[i][i - 2] = 0;
                    if (i > im_ + 2) T[i][i - 3] = 0;
                }
            }
        }
    }
    ltpo_schur_iterations = total_iter;   /* diagnostic (tools/schur_iters.py): Francis steps of the last solve */
    if (total_iter > 30 * n && total_iter <= max_iters) ltpo_schur_flags |= LTPO_F_CONVERGED_LATE;
    if (total_iter > max_iters) { ltpo_schur_flags |= LTPO_F_NOT_CONVERGED; return 1; } /* Eigen: NoConvergence, eigenvalues undefined */

    /* RealSchur: m_matT *= scale */
    for (i = 0; i < n; i++) for (j = 0; j < n; j++) T[i][j] = T[i][j] * scale;

    /* EigenSolver::compute: eigenvalues from the quasi-triangular T */
    i = 0;
    while (i < n) {
        if (i == n - 1 || T[i + 1][i] == 0) {
            REAL e = T[i][i];
            if (!(e - e == 0)) { ltpo_schur_flags |= LTPO_F_NONFINITE_EIGENVALUE; return 2; } /* Eigen: NumericalIssue, rest undefined */
            re[i] = e;
            im[i] = 0;
            ++i;
        } else {
            REAL pp = (REAL)0.5 * (T[i][i] - T[i + 1][i + 1]);
            REAL t0 = T[i + 1][i], t1 = T[i][i + 1];
            REAL maxval = FN(rs_max)(FN(rs_abs)(pp), FN(rs_max)(FN(rs_abs)(t0), FN(rs_abs)(t1)));
            REAL p0, z, er;
            t0 /= maxval;
            t1 /= maxval;
            p0 = pp / maxval;
            z = maxval * REAL_SQRT(FN(rs_abs)(p0 * p0 + t0 * t1));
            er = T[i + 1][i + 1] + pp;
            if (!(er - er == 0) || !(z - z == 0)) { ltpo_schur_flags |= LTPO_F_NONFINITE_EIGENVALUE; return 2; }
            if (z == 0) ltpo_schur_flags |= LTPO_F_PAIR_Z_ZERO;
            re[i] = er; im[i] = z;
            re[i + 1] = er; im[i + 1] = -z;
            i += 2;
        }
    }
    return 0;
}

/* roots.h:43-50: min{ re : im == 0 && re > 1e-7 }, else +INFINITY */
static REAL FN(smallest_positive_real_root)(const REAL *re, const REAL *im, int n)
{
    REAL best = (REAL)INFINITY;
    int i;
    for (i = 0; i < n; i++) {
        if (im[i] == 0 && re[i] > 1e-7) best = (re[i] < best) ? re[i] : best;
    }
    return best;
}
