// openwurli-hip: the pump-dynamics fitter of tools/analyze_pump_dynamics.py on the device (gfx950, f64): six cheap predictors
// R(t) -> pump(t) over a static pump table, their RMSE against a captured trace, and scipy's non-adaptive Nelder-Mead over them.
//
//   k_pump_fit_lut    one block: ln(lut_r) by the device's log and the table's slopes (numpy.interp's: (v[j+1] - v[j]) / (x[j+1] - x[j])).
//                     The knots' logarithms and those of the samples come from the same function, so a sample on a knot finds it.
//   k_pump_fit_prep   thread = sample: ln R[n] and the table's value at R[n], which every evaluation on that trace shares.
//   k_pump_fit_eval   lane = evaluation; a wavefront holds up to 64 evaluations of one (trace, model).
//   k_pump_fit        a wavefront holds up to 8 fits of one (trace, model); a fit owns a row of 8 lanes.  One pass over the trace
//                     evaluates the start simplex (N + 1 <= 5 lanes), and afterwards one pass per iteration evaluates everything the
//                     iteration can ask for: reflection, expansion, outside and inside contraction, and the N <= 4 shrink vertices --
//                     all affine in the ordered simplex, so all known before any loss is.  The row's first lane then takes scipy's
//                     decision from the eight losses (the simplex lives in LDS) and counts nfev as scipy would have.  A finished fit
//                     idles (its lanes keep evaluating their last candidates) until every fit of the wavefront is done.
//
// The sample loop (pf_pass) is the only expensive part.  The trace, model and length are wave-uniform -- read from a record indexed by
// blockIdx -- so R[n], ln R[n], the table's value and the target arrive through scalar loads, OW_PF_CHUNK samples per trip requested
// together at its head; the lanes differ in their parameters only and run the same instructions.  The two low-pass models look the table up per lane and sample: a lane keeps the interval it is in
// (knots, value, slope) in registers and the wavefront repeats the fixed-length binary search (over LDS) only at a sample where some lane
// left its interval: a wave-uniform branch on a ballot.  A lane's numbers never depend on the other lanes: the search it is dragged
// through returns the interval it already had.
//
// Arithmetic: every operation that the reference states is one IEEE operation here (__dmul_rn / __dadd_rn / __dsub_rn: never
// contracted), in the reference's order; division and square root are the correctly rounded ones.  exp and log are the device
// library's (within an ulp of the host's).  The loss sums d * d in sample order in the lane.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace owdev {

#define OW_PF_MAX_LUT 1024       // table points held in LDS (3 x 8 KB)
#define OW_PF_ROWS 8             // fits per wavefront
#define OW_PF_LANES 8            // lanes per fit: xr, xe, xc, xcc and up to four shrink vertices
#define OW_PF_MAX_PARAMS 4
#define OW_PF_CHUNK 8             // samples per trip of the sample loop
#define OW_PF_INVALID 1e9        // the reference's loss for a prediction that is not finite everywhere

struct OwPfTraceDev {
    uint64_t off;                // first sample in the concatenated arrays
    uint32_t n, pad;
    double sr;
};
struct OwPfWaveDev {             // one wavefront's share of the sorted list
    uint32_t trace, model, first, count;
};
struct OwPfLut {                 // in LDS
    const double* ln;
    const double* v;
    const double* slope;
    int n, steps;                // steps = ceil(log2(n)): the binary search's fixed length
    double r_lo, r_hi;
};

__device__ inline int pf_n_params(uint32_t model) { return model < 2 ? 1 : model < 4 ? 2 : model == 4 ? 3 : 4; }
__device__ inline bool pf_finite(double x) { return fabs(x) < __longlong_as_double(0x7FF0000000000000ll); }
__device__ inline double pf_nan() { return __longlong_as_double(0x7FF8000000000000ll); }

struct PfInterval {              // numpy.interp's answer around one abscissa, kept while the abscissa stays inside [lo, hi)
    double lo, hi, v0, v1, slope;
    bool flat;                   // left of the table, on its last knot or right of it: v0
};

// the interval of lx: the last j with ln[j] <= lx by a search of fixed length (indices stay inside the table whatever lx is)
__device__ inline void pf_search(const OwPfLut& t, double lx, PfInterval& c) {
    const double inf = __longlong_as_double(0x7FF0000000000000ll);
    int lo = 0, hi = t.n - 1;
    for (int s = 0; s < t.steps; ++s) {
        const int mid = (lo + hi + 1) >> 1;
        const bool le = t.ln[mid] <= lx;
        lo = le ? mid : lo;
        hi = le ? hi : mid - 1;
    }
    const int j = lo, last = t.n - 1;
    const int j1 = j < last ? j + 1 : last;
    const bool left = lx < t.ln[0], right = lx > t.ln[last] || j == last;
    c.flat = left || right;
    c.lo = left ? -inf : t.ln[right ? last : j];
    c.hi = left ? t.ln[0] : right ? inf : t.ln[j1];
    c.v0 = left ? t.v[0] : t.v[right ? last : j];
    c.v1 = t.v[j1];
    c.slope = t.slope[j < last ? j : 0];
}
__device__ inline bool pf_inside(const PfInterval& c, double lx) { return lx >= c.lo && lx < c.hi; }
__device__ inline double pf_value(const PfInterval& c, double lx) {
    double out = __dadd_rn(__dmul_rn(c.slope, __dsub_rn(lx, c.lo)), c.v0);
    if (out != out) {                                        // numpy.interp: "if we get nan in one direction, try the other"
        out = __dadd_rn(__dmul_rn(c.slope, __dsub_rn(lx, c.hi)), c.v1);
        if (out != out && c.v0 == c.v1) out = c.v0;
    }
    out = (c.flat || lx == c.lo) ? c.v0 : out;
    return lx != lx ? lx : out;
}
// ln(clip(x, r[0], r[-1])): a NaN passes through, as through np.clip
__device__ inline double pf_abscissa(const OwPfLut& t, double x) {
    const double c = x < t.r_lo ? t.r_lo : (x > t.r_hi ? t.r_hi : x);
    return log(c);
}
// the whole lookup, for code outside the sample loop
__device__ inline double pf_lookup(const OwPfLut& t, double x) {
    const double lx = pf_abscissa(t, x);
    PfInterval c;
    pf_search(t, lx, c);
    return pf_value(c, lx);
}

// the reference's guards: false where it returns a row of NaN without running
__device__ inline bool pf_valid(uint32_t model, double p0, double p1) {
    if (model < 2) return !(p0 <= 0.0);
    if (model < 5) return p0 >= 0.0 && p0 < 1.0;
    const double disc = __dadd_rn(__dmul_rn(p0, p0), __dmul_rn(4.0, p1));
    if (disc >= 0.0) {
        const double sq = __dsqrt_rn(disc);
        const double z1 = __dmul_rn(0.5, __dadd_rn(p0, sq)), z2 = __dmul_rn(0.5, __dsub_rn(p0, sq));
        return !(fabs(z1) >= 1.0 || fabs(z2) >= 1.0);
    }
    return !(__dsqrt_rn(-p1) >= 1.0);
}

// One evaluation in one lane: the loss of (model M, p0..p3) on the trace.  R / LN / BASE / TGT are wave-uniform pointers.
// PRED: the prediction row goes to pred[0 .. n).
template <int M, bool PRED>
__device__ inline double pf_pass(const double* __restrict__ R, const double* __restrict__ LN, const double* __restrict__ BASE,
                                 const double* __restrict__ TGT, uint32_t n, uint32_t skip, double sr, double p0, double p1, double p2, double p3,
                                 const OwPfLut& lut, double* __restrict__ pred) {
    const bool ok = pf_valid(M, p0, p1);
    if (!ok) { p0 = M < 2 ? 1.0 : 0.0; p1 = 0.0; p2 = 0.0; p3 = 0.0; }      // an invalid lane runs along on harmless numbers
    bool bad = false;
    double acc = 0.0;
    double s = 0.0, x1 = 0.0, x2 = 0.0, a = 0.0;
    PfInterval iv;
    auto emit = [&](uint32_t k, double y, bool count, double tk) {      // tk: the target at k where the sample counts
        bad = bad || !pf_finite(y);
        if (PRED) pred[k] = ok ? y : pf_nan();
        if (count) {
            const double d = __dsub_rn(y, tk);
            acc = __dadd_rn(acc, __dmul_rn(d, d));
        }
    };
    auto table_at = [&](double x) {                          // lpf models: the lookup through the kept interval
        const double lx = pf_abscissa(lut, x);
        if (__any(!pf_inside(iv, lx) && !bad)) pf_search(lut, lx, iv);   // wave-uniform; a lane inside its interval gets it again
        return pf_value(iv, lx);
    };
    // one sample from its operands: x0 = X[k], xm1 = X[k-1], xm2 = X[k-2] of the model's drive X (R or ln R), the table's value at R[k]
    auto advance = [&](uint32_t k, double x0, double xm1, double xm2, double bk, bool count, double tk) {
        double y;
        if (M < 2) {
            s = __dadd_rn(s, __dmul_rn(a, __dsub_rn(x0, s)));
            y = table_at(M == 0 ? s : exp(s));
        } else if (M < 4) {
            s = __dadd_rn(__dmul_rn(p0, s), __dmul_rn(p1, __dsub_rn(x0, xm1)));
            y = __dadd_rn(bk, s);
        } else if (M == 4) {
            const double du = __dsub_rn(x0, xm1);
            s = __dadd_rn(__dmul_rn(p0, s), __dmul_rn(du > 0.0 ? p1 : p2, du));
            y = __dadd_rn(bk, s);
        } else {
            const double u = __dsub_rn(x0, xm1), u1 = __dsub_rn(xm1, xm2);
            const double xi = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(p0, x1), __dmul_rn(p1, x2)), __dmul_rn(p2, u)), __dmul_rn(p3, u1));
            x2 = x1; x1 = xi;
            y = __dadd_rn(bk, xi);
        }
        emit(k, y, count, tk);
    };
    const double* __restrict__ X = (M == 0 || M == 2) ? R : LN;
    constexpr uint32_t BACK = M == 5 ? 2 : (M >= 2 ? 1 : 0);  // how far behind k the recurrence reads its drive
    auto step = [&](uint32_t k, bool count) {
        advance(k, X[k], BACK >= 1 ? X[k - 1] : 0.0, BACK >= 2 ? X[k - 2] : 0.0, M >= 2 ? BASE[k] : 0.0, count, count ? TGT[k] : 0.0);
    };
    // the samples the recurrences start from
    uint32_t k0;
    if (M < 2) {
        a = __dsub_rn(1.0, exp(-1.0 / __dmul_rn(__dmul_rn(sr, p0), 1e-3)));
        s = M == 0 ? R[0] : LN[0];
        const double lx = pf_abscissa(lut, M == 0 ? s : exp(s));
        pf_search(lut, lx, iv);
        emit(0, pf_value(iv, lx), skip == 0, TGT[0]);
        k0 = 1;
    } else if (M < 5) {
        emit(0, __dadd_rn(BASE[0], 0.0), skip == 0, TGT[0]);
        k0 = 1;
    } else {
        emit(0, __dadd_rn(BASE[0], 0.0), skip == 0, TGT[0]);
        emit(1, __dadd_rn(BASE[1], 0.0), skip <= 1, TGT[1]);
        k0 = 2;
    }
    uint32_t k = k0;
    for (; k < skip; ++k) step(k, false);                    // n > skip + 1: the host refuses shorter traces
    // eight samples per trip: their wave-uniform operands are requested together at the head of the trip and sit in SGPRs; the
    // scheduler may not sink a request into the arithmetic that would then wait for it
    for (; k + OW_PF_CHUNK <= n; k += OW_PF_CHUNK) {
        double xv[OW_PF_CHUNK + BACK], bv[OW_PF_CHUNK], tv[OW_PF_CHUNK];
#pragma unroll
        for (uint32_t j = 0; j < OW_PF_CHUNK + BACK; ++j) xv[j] = X[k - BACK + j];
#pragma unroll
        for (uint32_t j = 0; j < OW_PF_CHUNK; ++j) { bv[j] = M >= 2 ? BASE[k + j] : 0.0; tv[j] = TGT[k + j]; }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (uint32_t j = 0; j < OW_PF_CHUNK; ++j)
            advance(k + j, xv[j + BACK], BACK >= 1 ? xv[j + BACK - 1] : 0.0, BACK >= 2 ? xv[j] : 0.0, bv[j], true, tv[j]);
    }
    for (; k < n; ++k) step(k, true);
    if (!ok || bad) return OW_PF_INVALID;
    return __dmul_rn(1000.0, __dsqrt_rn(acc / (double)(n - skip)));
}

template <bool PRED>
__device__ inline double pf_dispatch(uint32_t model, const double* R, const double* LN, const double* BASE, const double* TGT, uint32_t n, uint32_t skip,
                                     double sr, double p0, double p1, double p2, double p3, const OwPfLut& lut, double* pred) {
    switch (model) {                                         // wave-uniform
        case 0: return pf_pass<0, PRED>(R, LN, BASE, TGT, n, skip, sr, p0, p1, p2, p3, lut, pred);
        case 1: return pf_pass<1, PRED>(R, LN, BASE, TGT, n, skip, sr, p0, p1, p2, p3, lut, pred);
        case 2: return pf_pass<2, PRED>(R, LN, BASE, TGT, n, skip, sr, p0, p1, p2, p3, lut, pred);
        case 3: return pf_pass<3, PRED>(R, LN, BASE, TGT, n, skip, sr, p0, p1, p2, p3, lut, pred);
        case 4: return pf_pass<4, PRED>(R, LN, BASE, TGT, n, skip, sr, p0, p1, p2, p3, lut, pred);
        default: return pf_pass<5, PRED>(R, LN, BASE, TGT, n, skip, sr, p0, p1, p2, p3, lut, pred);
    }
}

__global__ __launch_bounds__(256) void k_pump_fit_lut(const double* __restrict__ lut_r, const double* __restrict__ lut_v, int n,
                                                      double* __restrict__ ln_out, double* __restrict__ slope_out) {
    __shared__ double ln[OW_PF_MAX_LUT];
    for (int i = threadIdx.x; i < n; i += 256) { ln[i] = log(lut_r[i]); ln_out[i] = ln[i]; }
    __syncthreads();
    for (int j = threadIdx.x; j + 1 < n; j += 256) slope_out[j] = (lut_v[j + 1] - lut_v[j]) / (ln[j + 1] - ln[j]);
}

// the table from global memory into the block's LDS; every thread of the block calls it
__device__ inline void pf_load_lut(OwPfLut& t, double* s_ln, double* s_v, double* s_slope, const double* __restrict__ g_ln, const double* __restrict__ g_v,
                                   const double* __restrict__ g_slope, const double* __restrict__ lut_r, int n) {
    for (int i = threadIdx.x; i < n; i += blockDim.x) { s_ln[i] = g_ln[i]; s_v[i] = g_v[i]; s_slope[i] = i + 1 < n ? g_slope[i] : 0.0; }
    __syncthreads();
    t.ln = s_ln; t.v = s_v; t.slope = s_slope; t.n = n;
    t.steps = 32 - __clz(n - 1);                             // n >= 2
    t.r_lo = lut_r[0]; t.r_hi = lut_r[n - 1];
}

__global__ __launch_bounds__(256) void k_pump_fit_prep(const double* __restrict__ r, uint64_t total, const double* __restrict__ g_ln,
                                                       const double* __restrict__ g_v, const double* __restrict__ g_slope,
                                                       const double* __restrict__ lut_r, int n_lut, double* __restrict__ ln_out, double* __restrict__ base_out) {
    __shared__ double s_ln[OW_PF_MAX_LUT], s_v[OW_PF_MAX_LUT], s_slope[OW_PF_MAX_LUT];
    OwPfLut lut;
    pf_load_lut(lut, s_ln, s_v, s_slope, g_ln, g_v, g_slope, lut_r, n_lut);
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    ln_out[i] = log(r[i]);
    base_out[i] = pf_lookup(lut, r[i]);
}

// params: [n][4] in the sorted order; dest[i]: where evaluation i's results go (the caller's index)
__global__ __launch_bounds__(64) void k_pump_fit_eval(const OwPfTraceDev* __restrict__ traces, const OwPfWaveDev* __restrict__ waves,
                                                      const double* __restrict__ params, const uint32_t* __restrict__ dest,
                                                      const double* __restrict__ r, const double* __restrict__ lnr, const double* __restrict__ base,
                                                      const double* __restrict__ tgt, const double* __restrict__ g_ln, const double* __restrict__ g_v,
                                                      const double* __restrict__ g_slope, const double* __restrict__ lut_r, int n_lut, uint32_t skip,
                                                      double* __restrict__ loss_out, double* __restrict__ pred_out, uint64_t pred_stride) {
    __shared__ double s_ln[OW_PF_MAX_LUT], s_v[OW_PF_MAX_LUT], s_slope[OW_PF_MAX_LUT];
    OwPfLut lut;
    pf_load_lut(lut, s_ln, s_v, s_slope, g_ln, g_v, g_slope, lut_r, n_lut);
    const OwPfWaveDev w = waves[blockIdx.x];                 // wave-uniform: blockIdx and kernel arguments only
    const OwPfTraceDev t = traces[w.trace];
    const uint32_t lane = threadIdx.x;
    const bool has = lane < w.count;
    const uint32_t e = w.first + (has ? lane : 0);           // an idle lane repeats the wavefront's first evaluation
    const double p0 = params[4 * e], p1 = params[4 * e + 1], p2 = params[4 * e + 2], p3 = params[4 * e + 3];
    const uint32_t d = dest[e];
    double loss;
    if (pred_out)
        loss = pf_dispatch<true>(w.model, r + t.off, lnr + t.off, base + t.off, tgt + t.off, t.n, skip, t.sr, p0, p1, p2, p3, lut, pred_out + (uint64_t)d * pred_stride);
    else
        loss = pf_dispatch<false>(w.model, r + t.off, lnr + t.off, base + t.off, tgt + t.off, t.n, skip, t.sr, p0, p1, p2, p3, lut, nullptr);
    if (has) loss_out[d] = loss;
}

enum { PF_CONVERGED = 0, PF_MAXITER = 1, PF_START_INVALID = 2 };

// x0: [n][4] in the sorted order; dest as above.  Outputs by the caller's index: x [n][4] (0 beyond the model's parameters), fun, nit,
// nfev, status.
__global__ __launch_bounds__(64) void k_pump_fit(const OwPfTraceDev* __restrict__ traces, const OwPfWaveDev* __restrict__ waves,
                                                 const double* __restrict__ x0, const uint32_t* __restrict__ dest, const double* __restrict__ r,
                                                 const double* __restrict__ lnr, const double* __restrict__ base, const double* __restrict__ tgt,
                                                 const double* __restrict__ g_ln, const double* __restrict__ g_v, const double* __restrict__ g_slope,
                                                 const double* __restrict__ lut_r, int n_lut, uint32_t skip, double xatol, double fatol, uint32_t maxiter,
                                                 double* __restrict__ x_out, double* __restrict__ fun_out, uint32_t* __restrict__ nit_out,
                                                 uint32_t* __restrict__ nfev_out, uint32_t* __restrict__ status_out) {
    __shared__ double s_ln[OW_PF_MAX_LUT], s_v[OW_PF_MAX_LUT], s_slope[OW_PF_MAX_LUT];
    __shared__ double sim[OW_PF_ROWS][OW_PF_MAX_PARAMS + 1][OW_PF_MAX_PARAMS], fsim[OW_PF_ROWS][OW_PF_MAX_PARAMS + 1];
    __shared__ double cand[OW_PF_ROWS][OW_PF_LANES][OW_PF_MAX_PARAMS], fcand[OW_PF_ROWS][OW_PF_LANES];
    __shared__ uint32_t s_nit[OW_PF_ROWS], s_nfev[OW_PF_ROWS], s_active[OW_PF_ROWS], s_status[OW_PF_ROWS], s_start_invalid[OW_PF_ROWS];
    OwPfLut lut;
    pf_load_lut(lut, s_ln, s_v, s_slope, g_ln, g_v, g_slope, lut_r, n_lut);
    const OwPfWaveDev w = waves[blockIdx.x];                 // wave-uniform
    const OwPfTraceDev t = traces[w.trace];
    const int N = pf_n_params(w.model);
    const uint32_t row = threadIdx.x / OW_PF_LANES, l = threadIdx.x % OW_PF_LANES;
    const bool has = row < w.count;
    const uint32_t f = w.first + (has ? row : 0);            // an idle row repeats the wavefront's first start
    const bool keeper = l == 0;                              // the row's bookkeeping lane

    // the start simplex: x0, then each coordinate scaled by 1.05 (0.00025 where it is zero); spare lanes repeat x0
    if (keeper) {
        for (int i = 0; i < OW_PF_LANES; ++i)
            for (int k = 0; k < OW_PF_MAX_PARAMS; ++k) {
                double v = k < N ? x0[4 * f + k] : 0.0;
                if (i >= 1 && i <= N && k == i - 1) v = v != 0.0 ? __dmul_rn(1.0 + 0.05, v) : 0.00025;
                cand[row][i][k] = v;
            }
        s_active[row] = has ? 1u : 0u;
        s_status[row] = PF_MAXITER; s_nit[row] = 1; s_nfev[row] = (uint32_t)N + 1u;
    }
    __syncthreads();
    auto pass = [&]() {
        const double loss = pf_dispatch<false>(w.model, r + t.off, lnr + t.off, base + t.off, tgt + t.off, t.n, skip, t.sr, cand[row][l][0], cand[row][l][1],
                                               cand[row][l][2], cand[row][l][3], lut, nullptr);
        fcand[row][l] = loss;
        __syncthreads();
    };
    // stable insertion sort of the row's simplex by loss (ties keep their order)
    auto order = [&]() {
        for (int i = 1; i <= N; ++i) {
            const double key = fsim[row][i];
            const double t0 = sim[row][i][0], t1 = sim[row][i][1], t2 = sim[row][i][2], t3 = sim[row][i][3];
            int j = i - 1;
            while (j >= 0 && fsim[row][j] > key) {
                fsim[row][j + 1] = fsim[row][j];
                for (int k = 0; k < OW_PF_MAX_PARAMS; ++k) sim[row][j + 1][k] = sim[row][j][k];
                --j;
            }
            fsim[row][j + 1] = key;
            sim[row][j + 1][0] = t0; sim[row][j + 1][1] = t1; sim[row][j + 1][2] = t2; sim[row][j + 1][3] = t3;
        }
    };
    auto take = [&](int i, int c) {                          // vertex i of the simplex becomes candidate c
        fsim[row][i] = fcand[row][c];
        for (int k = 0; k < OW_PF_MAX_PARAMS; ++k) sim[row][i][k] = cand[row][c][k];
    };
    pass();
    if (keeper && has) {
        bool all_invalid = true;
        for (int i = 0; i <= N; ++i) { take(i, i); all_invalid = all_invalid && fcand[row][i] == OW_PF_INVALID; }
        s_start_invalid[row] = all_invalid ? 1u : 0u;
        order();
    }
    for (;;) {
        if (keeper && s_active[row]) {
            // scipy's loop head: `while iterations < maxiter`, then its two termination tests (np.max: a NaN wins, and fails the test)
            double dx = 0.0, df = 0.0;
            for (int i = 1; i <= N; ++i) {
                for (int k = 0; k < N; ++k) {
                    const double v = fabs(__dsub_rn(sim[row][i][k], sim[row][0][k]));
                    dx = (v > dx || v != v) ? v : dx;
                }
                const double v = fabs(__dsub_rn(fsim[row][0], fsim[row][i]));
                df = (df != df) ? df : ((v > df || v != v) ? v : df);
            }
            if (s_nit[row] >= maxiter) { s_active[row] = 0; s_status[row] = PF_MAXITER; }
            else if (dx <= xatol && df <= fatol) { s_active[row] = 0; s_status[row] = PF_CONVERGED; }
            else {
                // every point the iteration can need, in scipy's operation order: xbar = (sum of the N best, in order) / N;
                // xr = 2 xbar - 1 last; xe = 3 xbar - 2 last; xc = 1.5 xbar - 0.5 last; xcc = 0.5 xbar + 0.5 last; shrink: best + 0.5 (v - best)
                for (int k = 0; k < OW_PF_MAX_PARAMS; ++k) {
                    double xr = 0.0, xe = 0.0, xc = 0.0, xcc = 0.0;
                    if (k < N) {
                        double sum = sim[row][0][k];
                        for (int i = 1; i < N; ++i) sum = __dadd_rn(sum, sim[row][i][k]);
                        const double xbar = sum / (double)N, last = sim[row][N][k];
                        xr = __dsub_rn(__dmul_rn(2.0, xbar), __dmul_rn(1.0, last));
                        xe = __dsub_rn(__dmul_rn(3.0, xbar), __dmul_rn(2.0, last));
                        xc = __dsub_rn(__dmul_rn(1.5, xbar), __dmul_rn(0.5, last));
                        xcc = __dadd_rn(__dmul_rn(0.5, xbar), __dmul_rn(0.5, last));
                    }
                    cand[row][0][k] = xr; cand[row][1][k] = xe; cand[row][2][k] = xc; cand[row][3][k] = xcc;
                    for (int j = 1; j <= OW_PF_MAX_PARAMS; ++j)
                        cand[row][3 + j][k] = (k < N && j <= N) ? __dadd_rn(sim[row][0][k], __dmul_rn(0.5, __dsub_rn(sim[row][j][k], sim[row][0][k]))) : xr;
                }
            }
        }
        __syncthreads();
        if (!__any(s_active[row] != 0)) break;               // one wavefront per block: the ballot covers it
        pass();
        if (keeper && s_active[row]) {
            const double fxr = fcand[row][0], fxe = fcand[row][1], fxc = fcand[row][2], fxcc = fcand[row][3];
            uint32_t nfev = s_nfev[row] + 1u;
            bool shrink = false;
            if (fxr < fsim[row][0]) {
                ++nfev;
                take(N, fxe < fxr ? 1 : 0);
            } else if (fxr < fsim[row][N - 1]) {
                take(N, 0);
            } else if (fxr < fsim[row][N]) {
                ++nfev;
                if (fxc <= fxr) take(N, 2); else shrink = true;
            } else {
                ++nfev;
                if (fxcc < fsim[row][N]) take(N, 3); else shrink = true;
            }
            if (shrink) {
                for (int j = 1; j <= N; ++j) take(j, 3 + j);
                nfev += (uint32_t)N;
            }
            s_nfev[row] = nfev;
            s_nit[row] += 1u;
            order();
        }
        __syncthreads();
    }
    if (keeper && has) {
        const uint32_t d = dest[f];
        for (int k = 0; k < OW_PF_MAX_PARAMS; ++k) x_out[4 * d + k] = k < N ? sim[row][0][k] : 0.0;
        fun_out[d] = fsim[row][0];
        nit_out[d] = s_nit[row]; nfev_out[d] = s_nfev[row];
        status_out[d] = (s_start_invalid[row] && fsim[row][0] == OW_PF_INVALID) ? (uint32_t)PF_START_INVALID : s_status[row];
    }
}

}  // namespace owdev
