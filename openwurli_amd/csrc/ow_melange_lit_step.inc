// openwurli-hip: the body of mel_process_lit (ow_melange_lit.h), included there once per entry point.  The including file defines
//   OW_MEL_LIT_NAME          the function's name
//   OW_MEL_LIT_MORE_PARAMS   nothing, or further parameters (with their leading comma)
//   OW_MEL_LIT_COUNT(c, f)   nothing, or a statement counting condition c in field f of a MelDiag
// so that the entry point without counters is, token for token, the function it always was.
__device__ inline double OW_MEL_LIT_NAME(MelSt& st, double input_in, const double (*__restrict__ an)[12], double an66, const double* __restrict__ S,
                                         const double kk[3][3], const double* nz, int nz_stride OW_MEL_LIT_MORE_PARAMS) {
    const double input = isfinite(input_in) ? clampd(input_in, -100.0, 100.0) : 0.0;
#pragma unroll
    for (int i = 0; i < 12; ++i) st.v[i] = st.v[i] + 1e-25 - 1e-25;
#pragma unroll
    for (int i = 0; i < 3; ++i) st.ip[i] = st.ip[i] + 1e-25 - 1e-25;
    const bool force_be = st.be_cooldown > 0u;
    if (st.be_cooldown > 0u) st.be_cooldown -= 1u;
    const double* v = st.v;
#define AN(i, j) an[i][j]
    double rhs[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 15.0};     // RHS_CONST (gen_preamp.rs:760-773); build_rhs :3041-3095
    rhs[0] += AN(0, 0) * v[0] + AN(0, 1) * v[1];
    rhs[1] += AN(1, 0) * v[0] + AN(1, 1) * v[1] + AN(1, 2) * v[2];
    rhs[2] += AN(2, 1) * v[1] + AN(2, 2) * v[2] + AN(2, 3) * v[3] + AN(2, 4) * v[4] + AN(2, 5) * v[5];
    rhs[3] += AN(3, 2) * v[2] + AN(3, 3) * v[3] + AN(3, 4) * v[4] + AN(3, 7) * v[7] + AN(3, 11) * v[11];
    rhs[4] += AN(4, 2) * v[2] + AN(4, 3) * v[3] + AN(4, 4) * v[4] + AN(4, 7) * v[7] + AN(4, 8) * v[8];
    rhs[5] += AN(5, 2) * v[2] + AN(5, 5) * v[5] + AN(5, 6) * v[6];
    rhs[6] += AN(6, 5) * v[5] + an66 * v[6] + AN(6, 10) * v[10];
    rhs[7] += AN(7, 3) * v[3] + AN(7, 4) * v[4] + AN(7, 7) * v[7] + AN(7, 10) * v[10];
    rhs[8] += AN(8, 4) * v[4] + AN(8, 8) * v[8] + AN(8, 9) * v[9];
    rhs[9] += AN(9, 8) * v[8] + AN(9, 9) * v[9];
    rhs[10] += AN(10, 6) * v[6] + AN(10, 7) * v[7] + AN(10, 10) * v[10];
#undef AN
    rhs[2] += PRE_N_I[0][2] * st.ip[0];
    rhs[2] += PRE_N_I[1][2] * st.ip[1];
    rhs[4] += PRE_N_I[1][4] * st.ip[1];
    rhs[4] += PRE_N_I[2][4] * st.ip[2];
    rhs[5] += PRE_N_I[1][5] * st.ip[1];
    rhs[7] += PRE_N_I[2][7] * st.ip[2];
    rhs[8] += PRE_N_I[2][8] * st.ip[2];
    rhs[0] += (input + st.input_prev) / PRE_INPUT_RESISTANCE;
    if (nz) nz_stamp(rhs, nz, nz_stride);
    double v_pred[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) {                                  // v_pred = S rhs, rows in j order
        double sum = 0.0;
#pragma unroll
        for (int j = 0; j < 12; ++j) sum += MS(i, j) * rhs[j];
        v_pred[i] = sum;
    }
    const double p[3] = {-v_pred[2], v_pred[2] - v_pred[5], v_pred[4] - v_pred[8]};
    double i_nl[3];
    uint32_t last_it = mel_solve_nl(p, kk, st.ip, st.ipp, i_nl);
    // (fence: the S entries below were all read for S rhs above; without it the compiler keeps those 60 doubles in registers across
    // the Newton solve -- and spills -- instead of reading LDS again)
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    double vn[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) {                                  // v = v_pred + (S N_i) i_nl
        double x = v_pred[i];
        x += SNI0(i) * i_nl[0];
        x += SNI1(i) * i_nl[1];
        x += SNI2(i) * i_nl[2];
        vn[i] = x;
    }
    const bool nr_failed = last_it >= 265u;
    bool ringing = false;
#pragma unroll
    for (int i = 0; i < 11; ++i) ringing = ringing || (fabs(vn[i]) > 55.0);
    if (__builtin_expect(nr_failed || ringing || force_be, 0)) {
        OW_MEL_LIT_COUNT(nr_failed, nr_exhausted)                   // diag_nr_max_iter_count, the first of its two places (:3488)
        if (ringing || nr_failed) st.be_cooldown = 64u;
        st.be_fallbacks += 1u;
        MelSt tmp = st;
        double vn2[12], inl2[3];
        last_it = mel_be_fallback(tmp, input, vn2, inl2, nz, nz_stride);
#pragma unroll
        for (int i = 0; i < 12; ++i) vn[i] = vn2[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) i_nl[i] = inl2[i];
    }
    {   // voltage-damp net (gen_preamp.rs:3576-3613)
        double max_delta = 0.0;
#pragma unroll
        for (int i = 0; i < 11; ++i) { const double d = fabs(vn[i] - st.v[i]); if (d > max_delta) max_delta = d; }
        double max_dc = 0.0;
#pragma unroll
        for (int i = 0; i < 11; ++i) { const double a = fabs(PRE_DC_OP[i]); if (a > max_dc) max_dc = a; }
        const double thr = fma(max_dc, 0.05, 2.0);
        if (max_delta > thr) {
            OW_MEL_LIT_COUNT(true, voltage_damps)                   // diag_voltage_damp_count (:3599)
            const double damp = fmax(ow_div(thr, max_delta), 0.01);
#pragma unroll
            for (int i = 0; i < 12; ++i) vn[i] = st.v[i] + damp * (vn[i] - st.v[i]);
#pragma unroll
            for (int i = 0; i < 3; ++i) i_nl[i] = st.ip[i] + damp * (i_nl[i] - st.ip[i]);
        }
    }
    bool finite = true;
#pragma unroll
    for (int i = 0; i < 12; ++i) finite = finite && isfinite(vn[i]);
    if (!finite) {
#pragma unroll
        for (int i = 0; i < 12; ++i) st.v[i] = PRE_DC_OP[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) { st.ip[i] = PRE_DC_NL_I[i]; st.ipp[i] = PRE_DC_NL_I[i]; }
        st.input_prev = 0.0;
        st.pot = 9.99999999999999854e4;
        st.be_cooldown = 0u;
        st.nan_resets += 1u;
        return clampd(PRE_DC_OP[10] * 1.0, -10.0, 10.0);
    }
#pragma unroll
    for (int i = 0; i < 12; ++i) st.v[i] = vn[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) { st.ipp[i] = st.ip[i]; st.ip[i] = i_nl[i]; }
    st.input_prev = input;
    OW_MEL_LIT_COUNT(last_it >= 265u, nr_exhausted)                 // ... and the second, on the solve whose result is kept (:3647)
    const double raw = isfinite(vn[10]) ? vn[10] : 0.0;
    return raw * 1.0;
}
