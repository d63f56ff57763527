// spx_dual_step.inc — the body of k_dual_step, included by spx_dual.hip once
// per leaving-row rule with
//   SPX_STEP_KERNEL  the kernel's name
//   SPX_STEP_ARGS    DualArgs (Dantzig) or DualSeArgs (steepest edge)
//   SPX_STEP_SE      0 / 1
//   SPX_STEP_BOX     0 / 1 (1: SPX_STEP_ARGS is DualBoxArgs)
//   SPX_STEP_LONG    defined and 1 with SPX_STEP_BOX 1: SPX_STEP_ARGS is DualLongArgs
// Text inclusion, not a template: as a template instantiation (and as a
// forceinline body shared by two kernels) the Dantzig kernel compiled to a
// different schedule than the plain function it has always been; included
// with SPX_STEP_SE 0 it is that function, token for token.
// SE: the commit also turns the pass's exact row norms wex and tau = B^-1 rho
// (k_dual_update<., SE>) into the weights of the basis after the pivot, D.w,
// and the leaving row is the argmin of -x_b^2 / w.
// BOX (0 <= x <= u): a row leaves when x_b < -feas_tol (to its lower bound, s =
// +1) or x_b > u + feas_tol (to its upper bound, s = -1); delta is the violation
// on that side and takes x_b's place in both rules and in theta.  The side
// travels through the argmin in the row index's low bit (2 i + side: the order
// of the rows, hence the first index on ties, is kept, and the reduction is the
// unboxed one), the selection leaves s in the pass record, the commit forms
// delta_q from x_b[q] and ub_B[q] (loaded beside alpha_q: no longer chain),
// offsets the entering value by u_p when p sat at its upper bound and keeps
// at_upper / ub_B with the basis.
// LONG (the bound-flipping ratio test): when the pass flipped columns (nflip >
// 0) the commit works on x_b - fl, fl = B^-1 v loaded with the chunk's other
// vectors; delta_q comes from x_b[q] - fl_q.  Without a flip fl is not read and
// every value is the boxed kernel's.
__global__ __launch_bounds__(1024) void SPX_STEP_KERNEL(Params P, SPX_STEP_ARGS D, int finish_only) {
    constexpr int BLOCK = 1024, WAVES = BLOCK / 64;
    DevState* st = P.st;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t m = P.m, L = P.L;
    __shared__ StepState S;
    __shared__ ArgMinEntry s_red[WAVES];
#if SPX_STEP_LONG
    __shared__ int32_t s_nfl;  // the pass's flip count, read with the snapshot
#endif
    // The kernel is a chain of dependent memory round trips on one CU, so each
    // phase requests everything it needs before its first store: the state and
    // the pass record in one snapshot, the vectors in chunks of CH per thread
    // (loads of a chunk ahead of its stores), the bookkeeping's four loads
    // together on a wave of their own beside the vector updates.
    constexpr int CH = 4;
    if (tid == 0) {
        S.it = st->iter;
        S.limit = st->limit;
        S.qprev = st->q;
        S.aqprev = st->aq;
        S.status = st->status;
        S.y_buf = st->y_buf;
        S.cnt = st->nb_count;
        S.fresh = D.rec->fresh;
        S.q = D.rec->q;
        S.p = D.rec->p;
        S.d_p = D.rec->d_p;
#if SPX_STEP_LONG
        s_nfl = D.lrec->nflip;
#endif
    }
    __syncthreads();
    double* y = S.y_buf ? P.y1 : P.y0;
    int64_t it = S.it, qprev = S.qprev;
    double aqprev = S.aqprev;
    if (S.fresh) {
        // pivot it: alpha = B^-1 A_p is in alpha[(it + 1) & 1] (k_dual_update)
        const int64_t q = S.q, p = S.p;
        const double* al = ((it + 1) & 1) ? P.alpha1 : P.alpha0;
#if SPX_STEP_BOX
#if SPX_STEP_LONG
        const bool flp = s_nfl > 0;
        const double aq = al[q], xq0 = flp ? P.x_b[q] - D.fl[q] : P.x_b[q], ubq = D.ub_B[q];
#else
        const double aq = al[q], xq0 = P.x_b[q], ubq = D.ub_B[q];  // (every thread: the same words)
#endif
        const int32_t sgn = D.rec->s;
        const double xq = sgn > 0 ? xq0 : xq0 - ubq;  // delta_q
        const double u_p = D.ub[p];
        const double x_off = D.at_upper[p] ? u_p : 0.0;  // where the entering column starts from
#else
        const double aq = al[q], xq = P.x_b[q];  // (every thread: the same two words)
#endif
#if SPX_STEP_SE
        const double wq = D.tau[q];  // rho . rho
#endif
        const bool book = tid == BLOCK - 64;      // the last wave's lane 0
        int64_t leave = -1;
        double c_p = 0.0;
        int kp = -1, last = -1;
        if (book) {
            leave = P.b_ixs[q];
            c_p = P.c[p];
            kp = P.nb_pos[p];
            last = P.nb_list[S.cnt - 1];
        }
        const double theta = xq / aq, sy = -(S.d_p / aq);
        __syncthreads();  // x_b[q] is read by every thread before its owner overwrites it
        for (int64_t i0 = tid; i0 < L; i0 += (int64_t)CH * BLOCK) {
            double xv[CH], av[CH], yv[CH], rv[CH];
#if SPX_STEP_SE
            double ev[CH], tv[CH];
#endif
#pragma unroll
            for (int u = 0; u < CH; ++u) {
                const int64_t i = i0 + (int64_t)u * BLOCK;
                xv[u] = i < m ? P.x_b[i] : 0.0;
                av[u] = i < m ? al[i] : 0.0;
                yv[u] = i < L ? y[i] : 0.0;
                rv[u] = i < L ? D.rho[i] : 0.0;  // (rho's padding is 0: so is y's)
#if SPX_STEP_SE
                ev[u] = i < m ? D.wex[i] : 0.0;
                tv[u] = i < m ? D.tau[i] : 0.0;
#endif
#if SPX_STEP_LONG
                if (flp && i < m) xv[u] -= D.fl[i];
#endif
            }
#pragma unroll
            for (int u = 0; u < CH; ++u) {
                const int64_t i = i0 + (int64_t)u * BLOCK;
#if SPX_STEP_BOX
                if (i < m) P.x_b[i] = (i == q) ? x_off + theta : fma(-theta, av[u], xv[u]);
#else
                if (i < m) P.x_b[i] = (i == q) ? theta : fma(-theta, av[u], xv[u]);
#endif
                if (i < L) y[i] = fma(sy, rv[u], yv[u]);
#if SPX_STEP_SE
                // w'_i = w_i - 2 r_i tau_i + r_i^2 w_q, r_i = alpha_i / alpha_q; w'_q = w_q / alpha_q^2
                const double r = av[u] / aq;
                const double wn = fma(r * r, wq, fma(-2.0 * r, tv[u], ev[u]));
                if (i < m) D.w[i] = (i == q) ? wq / (aq * aq) : fmax(wn, DUAL_W_FLOOR);
#endif
            }
        }
        if (book) {
            P.c_B[q] = c_p;
            P.b_ixs[q] = p;
#if SPX_STEP_BOX
            D.ub_B[q] = u_p;
            D.at_upper[p] = 0;
            D.at_upper[leave] = sgn < 0 ? 1 : 0;
#endif
            // nb_list / nb_pos as pivot_bookkeeping keeps them: swap-remove p, append the leaving column
            int cnt = S.cnt;
            P.nb_list[kp] = last;
            P.nb_pos[last] = kp;
            P.nb_pos[p] = -1;
            --cnt;
            P.nb_list[cnt] = (int32_t)leave;
            P.nb_pos[leave] = cnt;
            ++cnt;
            st->nb_count = cnt;
            st->aq = aq;
            st->s_y = sy;
            st->y_applied = it + 1;  // y and x_b are current: only B^-1 stays pending
            st->xb_applied = it + 1;
            st->p = p;
            st->q = q;
            st->min_e = S.d_p;
            st->iter = it + 1;
            record_pivot(P, it, p, q);
            D.rec->fresh = 0;
#if SPX_STEP_LONG
            D.lrec->nflip = 0;
#endif
        }
        it += 1;
        qprev = q;
        aqprev = aq;
        __syncthreads();  // x_b as this workgroup's threads left it
    }
    if (finish_only || S.status != ST_RUNNING || it >= S.limit) return;

    // leaving row: the most negative x_b below -feas_tol (SE: the smallest
    // -x_b^2 / w among them), first index on ties
    double bv = INFINITY;
    int64_t bi = INT64_MAX;
#if SPX_STEP_BOX
    for (int64_t i = tid; i < m; i += BLOCK) {
        const double x = P.x_b[i], ub = D.ub_B[i];
        const double dl = x < -D.feas_tol ? x : (x > ub + D.feas_tol ? x - ub : 0.0);
#if SPX_STEP_SE
        const double v = -(dl * dl) / D.w[i];
#else
        const double v = -fabs(dl);
#endif
        const int64_t i2 = 2 * i + (dl > 0.0 ? 1 : 0);  // (row, side)
        if (dl != 0.0 && argmin_better(v, i2, bv, bi)) {
            bv = v;
            bi = i2;
        }
    }
#else
    for (int64_t i = tid; i < m; i += BLOCK) {
#if SPX_STEP_SE
        const double x = P.x_b[i];
        const double v = -(x * x) / D.w[i];
        if (x < -D.feas_tol && argmin_better(v, i, bv, bi)) {
#else
        const double v = P.x_b[i];
        if (v < -D.feas_tol && argmin_better(v, i, bv, bi)) {
#endif
            bv = v;
            bi = i;
        }
    }
#endif
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double v2 = __shfl_xor(bv, off, 64);
        const int64_t j2 = __shfl_xor(bi, off, 64);
        if (argmin_better(v2, j2, bv, bi)) {
            bv = v2;
            bi = j2;
        }
    }
    if (lane == 0) s_red[wave] = ArgMinEntry{bv, bi};
    __syncthreads();
    if (tid == 0) {
        ArgMinEntry t = s_red[0];
        for (int w = 1; w < WAVES; ++w)
            if (argmin_better(s_red[w].val, s_red[w].idx, t.val, t.idx)) t = s_red[w];
#if SPX_STEP_BOX
        if (t.idx != INT64_MAX) {
            D.rec->s = (t.idx & 1) ? -1 : 1;
            t.idx >>= 1;
        }
#endif
        S.q = t.idx;
        if (t.idx == INT64_MAX) st->status = ST_OPTIMAL;  // primal feasible: optimum
        else D.rec->q = t.idx;
    }
    __syncthreads();
    const int64_t q = S.q;
    if (q == INT64_MAX) return;

    // rho = row q of the true B^-1 = S[q] + E_q r', r' = S[q'] the pending pivot's
    // row (staged into rbuf: k_dual_update overwrites row q' while other waves
    // still read it)
    const bool pend = it > 0 && qprev >= 0;
    const double* Sq = P.B0 + q * L;
    const double* Sp = P.B0 + (pend ? qprev : q) * L;
    const double* a_prev = (it & 1) ? P.alpha1 : P.alpha0;
    const double aq_prev = pend ? a_prev[q] : 0.0;
    for (int64_t k0 = tid; k0 < L; k0 += (int64_t)CH * BLOCK) {
        double sp[CH], sq[CH];
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            const int64_t k = k0 + (int64_t)u * BLOCK;
            sq[u] = k < L ? Sq[k] : 0.0;
            sp[u] = (pend && k < L) ? Sp[k] : 0.0;
        }
        const double eq = pend ? eta_entry(aq_prev, q, qprev, aqprev) : 0.0;
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            const int64_t k = k0 + (int64_t)u * BLOCK;
            if (k < L) {
                if (pend) P.rbuf[k] = sp[u];
                D.rho[k] = pend ? fma(eq, sp[u], sq[u]) : sq[u];
            }
        }
    }
}
