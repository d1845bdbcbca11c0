// openwurli-hip host side, part of openwurli_hip.hip (one translation unit): C-ABI of include/openwurli_hip_test.h: host-logic hooks, diagnostics, switches.
extern "C" {
// ---- host-logic test hooks (no device) -----------------------------------------------------------
ow_engine* ow_test_engine_new(double sample_rate) {
    ow_engine* e = new ow_engine();
    e->sr = sample_rate;
    return e;
}
void ow_test_engine_free(ow_engine* e) { if (e && !e->pool) delete e; }
size_t ow_test_engine_take_ops(ow_engine* e, uint8_t* type, uint8_t* slot, uint8_t* note, uint32_t* seed, double* velocity, size_t cap) {
    if (!e) return 0;
    const size_t n = std::min(cap, e->ops.size());
    for (size_t i = 0; i < n; ++i) {
        type[i] = e->ops[i].type; slot[i] = e->ops[i].slot; note[i] = e->ops[i].note; seed[i] = e->ops[i].seed; velocity[i] = e->ops[i].velocity;
    }
    const size_t total = e->ops.size();
    e->ops.clear();
    return total;
}
void ow_test_engine_after_render(ow_engine* e, size_t len, uint64_t silent_mask) {
    if (!e) return;
    OwEngineOut o;
    std::memset(&o, 0, sizeof o);
    o.silent_mask = silent_mask;
    engine_post_render(e, (uint32_t)std::min<size_t>(len, 0xFFFFFFFFull), o);
}
uint64_t ow_test_engine_masks(const ow_engine* e, int which) { return e ? (which ? e->vm->steal_mask : e->vm->main_mask) : 0; }
int ow_test_pool_stagger_tremolo(ow_pool* p, size_t n_groups) {
    if (!p || n_groups == 0 || n_groups > p->I) return -1;
    try {
        HIP_OK(hipSetDevice(p->device));
        invalidate_spec(p);
        HIP_OK(hipStreamSynchronize(p->stream));
        const uint32_t I = (uint32_t)p->I, G = (uint32_t)n_groups;
        const long long period0 = (long long)(p->hc.os_sr / 5.6);
        const long long step0 = std::max<long long>(1, period0 / (long long)G);
        if (p->traj) {
            // on the shared trajectory "group g runs g * step samples ahead" is a shift of its engines' births (from the pool's common t)
            if (p->n_on_traj != p->I) throw std::runtime_error("stagger: an engine has left the trajectory");
            const long long b0 = p->min_birth;
            for (uint32_t e = 0; e < I; ++e) p->h_birth[e] = b0 - (long long)(e % G) * step0;
            traj_upload_births(p, 0, (int)I);
            traj_recount(p);
            return 0;
        }
        // every engine takes the oscillator state of its current leader, then group g = {g, g + G, ...} is led by engine g
        size_t n_copy = 0;
        for (uint32_t g = 0; g < G; ++g) { p->h_copy[n_copy] = p->h_lead[g]; p->h_copy[I + n_copy] = g; ++n_copy; }
        HIP_OK(hipMemcpyAsync(p->d_copy, p->h_copy, sizeof(uint32_t) * n_copy, hipMemcpyHostToDevice, p->stream));
        HIP_OK(hipMemcpyAsync(p->d_copy + I, p->h_copy + I, sizeof(uint32_t) * n_copy, hipMemcpyHostToDevice, p->stream));
        // leaders of the old groups are among the sources: copy through the backup buffer so that no source row is overwritten first
        HIP_OK(hipMemcpyAsync(p->d_trem_backup, p->d_cs, sizeof(double) * 18 * p->I, hipMemcpyDeviceToDevice, p->stream));
        owdev::k_trem_copy_rows_from<<<dim3((unsigned)((n_copy + 63) / 64)), dim3(64), 0, p->stream>>>(p->d_cs, p->d_trem_backup, (int)I, p->d_copy, p->d_copy + I, (int)n_copy);
        for (uint32_t e = 0; e < I; ++e) p->h_lead[e] = e % G;
        trem_groups_changed(p);
        trem_leader_list(p, 0, (int)I);
        // group g runs g * step samples ahead of group 0; the steps cover one period of the ~5.6 Hz oscillator
        const long long period = (long long)(p->hc.os_sr / 5.6);
        const long long step = std::max<long long>(1, period / (long long)G);
        if (p->tremolo_kind == OW_TREMOLO_LEGACY_LFO)
            owdev::k_tremolo_lfo<<<dim3((p->n_lead + 63) / 64), dim3(64), 0, p->stream>>>(p->dK, p->d_cs, nullptr, (int)I, 0LL, p->d_leaders, p->n_lead, step);
        else
            owdev::k_trem_settle<<<dim3((p->n_lead + 63) / 64), dim3(64), 0, p->stream>>>(p->dK, p->d_cs, (int)I, p->d_leaders, p->n_lead, 0LL, step);
        HIP_OK(hipGetLastError());
        HIP_OK(hipStreamSynchronize(p->stream));
        return 0;
    } catch (const std::exception& ex) { set_err(std::string("ow_test_pool_stagger_tremolo: ") + ex.what()); return -1; }
}
size_t ow_test_pool_tremolo_groups(const ow_pool* p) {
    if (!p) return 0;
    size_t n = 0;
    if (p->traj) {       // distinct tremolo phases: engines on the trajectory share an oscillator exactly when they stand at the same t
        std::vector<long long> b;
        for (size_t e = 0; e < p->I; ++e) { if (p->h_birth[e] != OW_OFF_TRAJ) b.push_back(p->h_birth[e]); else n += p->h_lead[e] == (uint32_t)e; }
        std::sort(b.begin(), b.end());
        return n + (size_t)(std::unique(b.begin(), b.end()) - b.begin());
    }
    for (size_t e = 0; e < p->I; ++e) n += p->h_lead[e] == (uint32_t)e;
    return n;
}
int ow_debug_power_amp(double sample_rate, const double* in, size_t n_rows, size_t n, int rail_sag, const long long* poke_at, const int* poke_node,
                       const double* poke_val, double* out, double* taps, int device) {
    try {
        if (!in || !out || n_rows == 0 || n == 0 || !(sample_rate > 0.0)) throw std::runtime_error("bad argument");
        HIP_OK(hipSetDevice(device));
        StreamOwner so;
        so.create();
        std::unique_ptr<OwPaConsts> hc(new OwPaConsts());
        owhip::build_pa_consts(*hc, sample_rate);
        DevMem dC, dS, dIn, dOut, dT, dPa, dPn, dPv;
        dC.alloc(sizeof(OwPaConsts)); dS.alloc(sizeof(double) * owdev::PAS_CIRCUIT_END);
        dIn.alloc(sizeof(double) * n_rows * n); dOut.alloc(sizeof(double) * n_rows * n);
        if (taps) dT.alloc(sizeof(double) * n_rows * n * 3);
        pa_settled_to_device(device, dS.as<double>(), so.s);
        HIP_OK(hipMemcpyAsync(dC.p, hc.get(), sizeof(OwPaConsts), hipMemcpyHostToDevice, so.s));
        HIP_OK(hipMemcpyAsync(dIn.p, in, sizeof(double) * n_rows * n, hipMemcpyHostToDevice, so.s));
        if (poke_at) {
            dPa.alloc(sizeof(long long) * n_rows); dPn.alloc(sizeof(int) * n_rows); dPv.alloc(sizeof(double) * n_rows);
            HIP_OK(hipMemcpyAsync(dPa.p, poke_at, sizeof(long long) * n_rows, hipMemcpyHostToDevice, so.s));
            HIP_OK(hipMemcpyAsync(dPn.p, poke_node, sizeof(int) * n_rows, hipMemcpyHostToDevice, so.s));
            HIP_OK(hipMemcpyAsync(dPv.p, poke_val, sizeof(double) * n_rows, hipMemcpyHostToDevice, so.s));
        }
        owdev::k_mpa_debug<<<dim3((unsigned)((n_rows + PA_EPB - 1) / PA_EPB)), dim3(PA_WPB * 64), 0, so.s>>>(dC.as<OwPaConsts>(), dS.as<double>(), dIn.as<double>(), dOut.as<double>(),
                                                                          taps ? dT.as<double>() : nullptr, (long long)n, (int)n_rows, rail_sag,
                                                                          poke_at ? dPa.as<long long>() : nullptr, dPn.as<int>(), dPv.as<double>());
        HIP_OK(hipGetLastError());
        HIP_OK(hipMemcpyAsync(out, dOut.p, sizeof(double) * n_rows * n, hipMemcpyDeviceToHost, so.s));
        if (taps) HIP_OK(hipMemcpyAsync(taps, dT.p, sizeof(double) * n_rows * n * 3, hipMemcpyDeviceToHost, so.s));
        HIP_OK(hipStreamSynchronize(so.s));
        return 0;
    } catch (const std::exception& ex) { set_err(std::string("ow_debug_power_amp: ") + ex.what()); return -1; }
}
int ow_test_pool_power_amp_passes(ow_pool* p, uint32_t* out, size_t n) {
    if (!p || !out || !p->d_pa_demand || n != (size_t)p->I) return -1;
    if (hipSetDevice(p->device) != hipSuccess) return -1;
    if (hipStreamSynchronize(p->stream) != hipSuccess) return -1;
    return hipMemcpy(out, p->d_pa_demand, sizeof(uint32_t) * n, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
int ow_test_pool_enable_power_amp_tap(ow_pool* p) {
    if (!p || p->power_amp_kind != OW_POWER_AMP_MELANGE) return -1;
    if (p->d_pa_tap) return 0;
    if (hipSetDevice(p->device) != hipSuccess || hipStreamSynchronize(p->stream) != hipSuccess) return -1;
    try { p->d_pa_tap.alloc(2 * p->Lcap * p->I); return 0; } catch (const std::exception&) { return -1; }
}
int ow_test_pool_read_power_amp_out(ow_pool* p, double* out_host, size_t out_stride, size_t n_os) {
    if (!p || !out_host || !p->d_pa_tap || n_os > 2 * p->Lcap) return -1;
    try {
        HIP_OK(hipSetDevice(p->device));
        const size_t I = p->I;
        std::vector<double> a(I * n_os);
        HIP_OK(hipMemcpy(a.data(), p->d_pa_tap, sizeof(double) * I * n_os, hipMemcpyDeviceToHost));  // [n_os][I]
        for (size_t e = 0; e < I; ++e)
            for (size_t n = 0; n < n_os; ++n) out_host[e * out_stride + n] = a[n * I + e];
        return 0;
    } catch (const std::exception& ex) { set_err(std::string("ow_test_pool_read_power_amp_out: ") + ex.what()); return -1; }
}
int ow_test_engine_poke_power_amp_node(ow_engine* e, int node, double volts) {
    if (!e || !e->pool || e->pool->power_amp_kind != OW_POWER_AMP_MELANGE || node < 0 || node >= PA_N) return -1;
    ow_pool* p = e->pool;
    if (hipSetDevice(p->device) != hipSuccess || hipStreamSynchronize(p->stream) != hipSuccess) return -1;
    return hipMemcpy(p->d_pa + (size_t)(owdev::PAS_V + node) * p->I + e->index, &volts, sizeof volts, hipMemcpyHostToDevice) == hipSuccess ? 0 : -1;
}
// Host matrix builders (ow_consts_host.hpp) of the three generated solvers at `rate` (the solver's own rate: the chain rate), no device.
// force_rebuild != 0 bypasses the "codegen rate -> baked tables" shortcut so that the rebuild can be checked against those tables.
int ow_test_host_matrices(int solver, double rate, int force_rebuild, double* s, double* k, double* sni, double* aneg,
                          double* s_be, double* k_be, double* sni_be, double* aneg_be) {
    try {
        if (!(rate > 0.0)) throw std::runtime_error("bad rate");
        auto put = [](double* dst, const void* src, size_t n) { if (dst) std::memcpy(dst, src, sizeof(double) * n); };
        struct Force { Force(bool on) { owhip::g_force_rebuild = on; } ~Force() { owhip::g_force_rebuild = false; } } force(force_rebuild != 0);
        if (solver == 0 || solver == 1) {
            std::unique_ptr<OwConsts> c(new OwConsts());
            // build_consts takes the HOST rate; a host rate >= 88.2 kHz runs the chain at that rate without oversampling (engine.rs:195)
            owhip::build_consts(*c, rate < 88200.0 ? rate * 0.5 : rate, solver == 1 ? OW_PREAMP_MELANGE12 : OW_PREAMP_LEGACY8);
            if (c->os_sr != rate) throw std::runtime_error("rate is not reachable as a chain rate");
            if (solver == 0) {
                put(s, c->t_s, 49); put(k, c->t_k, 16); put(sni, c->t_s_ni, 28); put(aneg, c->t_a_neg, 49);
                put(s_be, c->t_s_be, 49); put(k_be, c->t_k_be, 16); put(sni_be, c->t_s_ni_be, 28); put(aneg_be, c->t_a_neg_be, 49);
                return 704;
            }
            put(s, c->m_s0, 144); put(k, c->m_k0, 9); put(sni, c->m_sni0, 36); put(aneg, c->m_aneg0, 144);
            // the melange preamp's backward-Euler set is never rebuilt (gen_preamp.rs:2058-2061): the kernels read the baked tables
            put(s_be, PRE_S_BE_DEFAULT, 144); put(k_be, PRE_K_BE_DEFAULT, 9); put(sni_be, PRE_S_NI_BE_DEFAULT, 36); put(aneg_be, PRE_A_NEG_BE_DEFAULT, 144);
            return 1203;
        }
        if (solver == 2) {
            std::unique_ptr<OwPaConsts> c(new OwPaConsts());
            owhip::build_pa_consts(*c, rate);
            put(s, c->s, 400); put(k, c->k, 256); put(sni, c->s_ni, 320); put(aneg, c->a_neg, 400);
            put(s_be, c->s_be, 400); put(k_be, c->k_be, 256); put(sni_be, c->s_ni_be, 320); put(aneg_be, c->a_neg_be, 400);
            return 2016;
        }
        throw std::runtime_error("unknown solver");
    } catch (const std::exception& ex) { set_err(std::string("ow_test_host_matrices: ") + ex.what()); return -1; }
}
// Forget the process-wide settled states (Twin-T per chain rate; melange preamp and power amp per device): the next pool settles
// afresh on the device.  Returns the number of cached Twin-T states that were dropped.
int ow_test_clear_settle_caches(void) {
    int n;
    {   // one lock at a time: traj_acquire holds g_traj_mu while its settle takes g_mel_mu (trem_settled_rows)
        std::lock_guard<std::mutex> lk(g_mel_mu);
        n = (int)g_trem_settled.size();
        g_trem_settled.clear(); g_mel_settled.clear(); g_pa_settled.clear();
    }
    { std::lock_guard<std::mutex> lt(g_traj_mu); traj_registry().clear(); }     // pools that hold a store keep it alive; new pools start a new one
    return n;
}
// Overwrite one field of a voice record (VF_* of ow_types.h) on the device before the next block: the way to make a voice non-finite,
// which no API call can (voice-sum NaN guard, engine.rs:496-521).
static_assert(VF_Q == OW_TEST_VF_Q && VF_S == OW_TEST_VF_S0, "openwurli_hip_test.h names two voice-record fields by index");
int ow_test_engine_poke_voice(ow_engine* e, int slot, int steal, int field, double value) {
    if (!e || !e->pool || slot < 0 || slot >= OW_MAX_VOICES || field < 0 || field >= VF_COUNT) return -1;
    ow_pool* p = e->pool;
    if (hipSetDevice(p->device) != hipSuccess || hipStreamSynchronize(p->stream) != hipSuccess) return -1;
    double* dst = p->d_vrec + ((size_t)e->index * 2 + (steal ? 1 : 0)) * OW_VREC_DOUBLES + (size_t)field * 64 + slot;
    return hipMemcpy(dst, &value, sizeof value, hipMemcpyHostToDevice) == hipSuccess ? 0 : -1;
}
// Overwrite one node voltage of the legacy preamp's main / shadow solver state before the next block: a non-finite one is how the preamp's
// own NaN reset (dk_preamp_legacy.rs:610-615: full DC solve at the current R_ldr, the sample's output 0) is provoked -- no API call can.
int ow_test_engine_poke_preamp_node(ow_engine* e, int shadow, int node, double volts) {
    if (!e || !e->pool || node < 0 || node >= 8) return -1;
    ow_pool* p = e->pool;
    if (p->hc.preamp_kind != OW_PREAMP_LEGACY8 || !p->d_cs) return -1;
    if (hipSetDevice(p->device) != hipSuccess || hipStreamSynchronize(p->stream) != hipSuccess) return -1;
    double* dst = p->d_cs + (size_t)((shadow ? CS_P_SHADOW : CS_P_MAIN) + 2 + node) * p->I + e->index;
    return hipMemcpy(dst, &volts, sizeof volts, hipMemcpyHostToDevice) == hipSuccess ? 0 : -1;
}
// ... and read the fourteen fields of that state back: j_cin, cin_rhs_prev, v[8], i_nl[2], v_nl[2] (DkState, dk_preamp_legacy.rs:231-239)
int ow_test_engine_read_preamp_state(ow_engine* e, int shadow, double* out14) {
    if (!e || !e->pool || !out14) return -1;
    ow_pool* p = e->pool;
    if (p->hc.preamp_kind != OW_PREAMP_LEGACY8 || !p->d_cs) return -1;
    if (hipSetDevice(p->device) != hipSuccess || hipStreamSynchronize(p->stream) != hipSuccess) return -1;
    for (int f = 0; f < 14; ++f) {
        const double* src = p->d_cs + (size_t)((shadow ? CS_P_SHADOW : CS_P_MAIN) + f) * p->I + e->index;
        if (hipMemcpy(out14 + f, src, sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    }
    return 0;
}
// Rows [first_row, first_row + n_rows) of engine e's chain state, cs[(first_row + i) * I + e], copied out / in as they stand: the whole
// output stage lives in rows CS_SM_SPK .. CS_SM_VOL, CS_OS_DA .. CS_SPK_TS and CS_FLAGS, so a test can start it from any state and read
// what a block left behind.  The write is a state change behind the scheduler's back, like ow_test_pool_set_switch.
static_assert(CS_SM_SPK == OW_TEST_CS_SM_SPK && CS_SM_VOL == OW_TEST_CS_SM_VOL && CS_OS_DA == OW_TEST_CS_OS_DA && CS_OS_DB == OW_TEST_CS_OS_DB &&
              CS_OS_DD == OW_TEST_CS_OS_DD && CS_SPK_HPF == OW_TEST_CS_SPK_HPF && CS_SPK_LPF == OW_TEST_CS_SPK_LPF &&
              CS_SPK_CHAR == OW_TEST_CS_SPK_CHAR && CS_SPK_A2 == OW_TEST_CS_SPK_A2 && CS_SPK_A3 == OW_TEST_CS_SPK_A3 &&
              CS_SPK_TC == OW_TEST_CS_SPK_TC && CS_SPK_TS == OW_TEST_CS_SPK_TS && CS_FLAGS == OW_TEST_CS_FLAGS && CS_COUNT == OW_TEST_CS_COUNT,
              "openwurli_hip_test.h names the output stage's chain-state rows by index");
int ow_test_engine_read_chain_rows(ow_engine* e, int first_row, int n_rows, double* out) {
    if (!e || !e->pool || !out || first_row < 0 || n_rows < 0 || first_row > CS_COUNT - n_rows) return -1;
    ow_pool* p = e->pool;
    if (!p->d_cs) return -1;
    if (n_rows == 0) return 0;
    if (hipSetDevice(p->device) != hipSuccess || hipStreamSynchronize(p->stream) != hipSuccess) return -1;
    const double* src = p->d_cs + (size_t)first_row * p->I + e->index;
    return hipMemcpy2D(out, sizeof(double), src, sizeof(double) * p->I, sizeof(double), (size_t)n_rows, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
int ow_test_engine_write_chain_rows(ow_engine* e, int first_row, int n_rows, const double* in) {
    if (!e || !e->pool || !in || first_row < 0 || n_rows < 0 || first_row > CS_COUNT - n_rows) return -1;
    ow_pool* p = e->pool;
    if (!p->d_cs) return -1;
    if (hipSetDevice(p->device) != hipSuccess) return -1;
    invalidate_spec(p);                                   // a pending block-ahead result was produced from the old rows
    if (hipStreamSynchronize(p->stream) != hipSuccess) return -1;
    if (n_rows == 0) return 0;
    double* dst = p->d_cs + (size_t)first_row * p->I + e->index;
    return hipMemcpy2D(dst, sizeof(double) * p->I, in, sizeof(double), sizeof(double), (size_t)n_rows, hipMemcpyHostToDevice) == hipSuccess ? 0 : -1;
}
// One whole voice record, vrec[e][steal][field][slot], copied out / in field-major (out[f] = field f of that slot; u64 fields as their
// bits): a voice block is a pure function (record, L) -> (record, L samples, status bits), and this is how a test starts it from any record
// and reads what it left.  The read shows the record as the last render left it: ops queued since are applied by the next one.
static_assert(VF_S == OW_TEST_VF_S0 && VF_C == OW_TEST_VF_C0 && VF_ENV == OW_TEST_VF_ENV0 && VF_DRIFT == OW_TEST_VF_DRIFT0 &&
              VF_COS_INC == OW_TEST_VF_COS_INC0 && VF_SIN_INC == OW_TEST_VF_SIN_INC0 && VF_PHASE_INC == OW_TEST_VF_PHASE_INC0 &&
              VF_AMP == OW_TEST_VF_AMP0 && VF_DECAY == OW_TEST_VF_DECAY0 && VF_DRATE == OW_TEST_VF_DRATE0 && VF_DMULT == OW_TEST_VF_DMULT0 &&
              VF_ONSET_INC == OW_TEST_VF_ONSET_INC && VF_ONSET_EXP == OW_TEST_VF_ONSET_EXP && VF_DRAMP == OW_TEST_VF_DRAMP &&
              VF_DCOUNT == OW_TEST_VF_DCOUNT && VF_Q == OW_TEST_VF_Q && VF_DS == OW_TEST_VF_DS && VF_GAIN == OW_TEST_VF_GAIN &&
              VF_NAMP == OW_TEST_VF_NAMP && VF_NB0 == OW_TEST_VF_NB0 && VF_NA2 == OW_TEST_VF_NB0 + 4 && VF_NS1 == OW_TEST_VF_NS1 &&
              VF_NS2 == OW_TEST_VF_NS2 && VF_SAMPLE == OW_TEST_VF_SAMPLE && VF_ONSET_N == OW_TEST_VF_ONSET_N && VF_RNG == OW_TEST_VF_RNG &&
              VF_NCNT == OW_TEST_VF_NCNT && VF_FLAGS == OW_TEST_VF_FLAGS && VF_STEAL == OW_TEST_VF_STEAL && VF_BETA == OW_TEST_VF_BETA &&
              VF_JREV == OW_TEST_VF_JREV && VF_JDIFF == OW_TEST_VF_JDIFF && VF_NDECAY == OW_TEST_VF_NDECAY && VF_VSR == OW_TEST_VF_VSR &&
              VF_COUNT == OW_TEST_VF_COUNT, "openwurli_hip_test.h names the voice record's fields by index");
int ow_test_engine_read_voice_record(ow_engine* e, int slot, int steal, double* out) {
    if (!e || !e->pool || !out || slot < 0 || slot >= OW_MAX_VOICES) return -1;
    ow_pool* p = e->pool;
    if (hipSetDevice(p->device) != hipSuccess || hipStreamSynchronize(p->stream) != hipSuccess) return -1;
    const double* src = p->d_vrec + ((size_t)e->index * 2 + (steal ? 1 : 0)) * OW_VREC_DOUBLES + slot;
    return hipMemcpy2D(out, sizeof(double), src, sizeof(double) * 64, sizeof(double), (size_t)VF_COUNT, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
// The write is a state change behind the scheduler's back, like ow_test_engine_write_chain_rows: a block rendered ahead is forgotten, the
// voice lists are packed again, and the engine's transient flag -- which of the voice kernels its slot voices get -- is what its sounding
// slot voices' records now say (VoiceRegs::in_transient: damper bit, sample < onset_n, noise remaining).  Which slots are occupied,
// releasing or stolen is the host's state machine and comes from the API calls alone.
int ow_test_engine_write_voice_record(ow_engine* e, int slot, int steal, const double* in) {
    if (!e || !e->pool || !in || slot < 0 || slot >= OW_MAX_VOICES) return -1;
    ow_pool* p = e->pool;
    if (hipSetDevice(p->device) != hipSuccess) return -1;
    invalidate_spec(p);
    if (hipStreamSynchronize(p->stream) != hipSuccess) return -1;
    vm_wait_download(p);                                  // the masks below are the host's copy
    double* rec0 = p->d_vrec + (size_t)e->index * 2 * OW_VREC_DOUBLES;
    if (hipMemcpy2D(rec0 + (steal ? OW_VREC_DOUBLES : 0) + slot, sizeof(double) * 64, in, sizeof(double), sizeof(double), (size_t)VF_COUNT,
                    hipMemcpyHostToDevice) != hipSuccess) return -1;
    std::vector<double> f(4 * 64);                        // VF_SAMPLE, VF_ONSET_N, VF_RNG, VF_NCNT of every slot voice ...
    double fl[64];                                        // ... and VF_FLAGS
    if (hipMemcpy(f.data(), rec0 + (size_t)VF_SAMPLE * 64, sizeof(double) * 4 * 64, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    if (hipMemcpy(fl, rec0 + (size_t)VF_FLAGS * 64, sizeof fl, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    static_assert(VF_ONSET_N == VF_SAMPLE + 1 && VF_NCNT == VF_SAMPLE + 3, "the four counters are read in one copy");
    auto bits = [](double d) { uint64_t u; std::memcpy(&u, &d, 8); return u; };
    uint8_t tr = 0;
    for (uint64_t m = e->vm->main_mask; m; m &= m - 1) {
        const int s = __builtin_ctzll(m);
        if ((bits(fl[s]) & 1ull) || bits(f[s]) < bits(f[64 + s]) || (uint32_t)bits(f[3 * 64 + s]) > 0u) tr = 1;
    }
    p->transient[e->index] = tr;
    p->lists_valid = false;
    if (p->d_prev_tr) p->attn_resync = true;              // p->transient moved without the device's copy
    return 0;
}
// plain device-to-host copy (tests read blocks that a render left in HBM: ow_pool_device_output)
int ow_test_device_read(void* dst_host, const void* src_device, size_t bytes, int device) {
    if (!dst_host || !src_device) return -1;
    if (hipSetDevice(device) != hipSuccess) return -1;
    return hipMemcpy(dst_host, src_device, bytes, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
// plain host-to-device copy (tests hand given audio to the audio_is_device paths)
int ow_test_device_write(void* dst_device, const void* src_host, size_t bytes, int device) {
    if (!dst_device || !src_host) return -1;
    if (hipSetDevice(device) != hipSuccess) return -1;
    return hipMemcpy(dst_device, src_host, bytes, hipMemcpyHostToDevice) == hipSuccess ? 0 : -1;
}
#ifdef OW_DBG_COUNTERS
// development counters (built with OW_HIPCC_EXTRA=-DOW_DBG_COUNTERS only): read and clear
extern "C" int ow_debug_counters(unsigned long long* out8, int device) {
    if (hipSetDevice(device) != hipSuccess) return -1;
    unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (hipMemcpyFromSymbol(out8, HIP_SYMBOL(owdev::g_ow_dbg), sizeof z) != hipSuccess) return -1;
    return hipMemcpyToSymbol(HIP_SYMBOL(owdev::g_ow_dbg), z, sizeof z) == hipSuccess ? 0 : -1;
}
#endif
// The two oscillator kernels of the shared trajectory on their own (no store, no pool): CircuitState at DC_OP, n_settle steps without
// the cell (Tremolo::new's settle), then n steps with it through a trajectory kernel in launches of `chunk` steps.  row = 0: the quad-lane
// kernels (k_tremolo_wide<true>, k_trem_traj_extend), 1: the row kernels (ow_trem_row.h).  r_out[n], state_out[18], ckpt_out[(n / 4096 + 2)
// * 16] (or NULL), be_out[1 + 1023] (or NULL); *ms_out = device time of the trajectory launches (HIP events).
int ow_debug_trem_trajectory(double sample_rate, long long n_settle, long long n, long long chunk, int row, double* r_out, double* state_out,
                             double* ckpt_out, unsigned long long* be_out, double* ms_out, int device, unsigned long long* cold_out, const double* kick18) {
    try {
        if (!r_out || !state_out || n <= 0 || n_settle < 0 || chunk <= 0) throw std::runtime_error("bad arguments");
        HIP_OK(hipSetDevice(device));
        std::unique_ptr<OwConsts> hc(new OwConsts());
        owhip::build_consts(*hc, sample_rate, OW_PREAMP_LEGACY8);
        DevMem dk, dstate, dr, dck, dbe, dzero;
        dk.alloc(sizeof(OwConsts)); dstate.alloc(sizeof(double) * 18); dr.alloc(sizeof(double) * (size_t)(n + 64));
        const size_t nck = TremTraj::ckpt_doubles((size_t)n);
        dck.alloc(sizeof(double) * nck); dbe.alloc(sizeof(unsigned long long) * (1 + OW_TRAJ_BE_CAP)); dzero.alloc(sizeof(uint32_t));
        StreamOwner so;
        so.create(hipStreamDefault);
        HIP_OK(hipMemcpyAsync(dk.p, hc.get(), sizeof(OwConsts), hipMemcpyHostToDevice, so.s));
        HIP_OK(hipMemsetAsync(dck.p, 0, sizeof(double) * nck, so.s));
        HIP_OK(hipMemsetAsync(dbe.p, 0xFF, sizeof(unsigned long long) * (1 + OW_TRAJ_BE_CAP), so.s));
        HIP_OK(hipMemsetAsync(dbe.p, 0, sizeof(unsigned long long), so.s));
        HIP_OK(hipMemsetAsync(dzero.p, 0, sizeof(uint32_t), so.s));
        owdev::k_trem_state_dc<<<dim3(1), dim3(64), 0, so.s>>>(dstate.as<double>());
        if (kick18) {          // the circuit pushed off its operating point (added to rows 0..14: v, i_prev, i_pp): the limiter, the step cap, other pivots
            double rows[18];
            HIP_OK(hipMemcpyAsync(rows, dstate.p, sizeof rows, hipMemcpyDeviceToHost, so.s));
            HIP_OK(hipStreamSynchronize(so.s));
            for (int i = 0; i < 15; ++i) rows[i] += kick18[i];
            HIP_OK(hipMemcpyAsync(dstate.p, rows, sizeof rows, hipMemcpyHostToDevice, so.s));
            HIP_OK(hipStreamSynchronize(so.s));
        }
        if (n_settle > 0) {
            if (row) owdev::k_trem_settle_row<<<dim3(1), dim3(64), 0, so.s>>>(dk.as<OwConsts>(), dstate.as<double>(), n_settle);
            else owdev::k_tremolo_wide<true><<<dim3(1), dim3(64), 0, so.s>>>(dk.as<OwConsts>(), dstate.as<double>(), nullptr, 1, n_settle, dzero.as<uint32_t>(), 1);
        }
        unsigned long long cold0[2] = {0, 0}, cold1[2] = {0, 0};
        HIP_OK(hipStreamSynchronize(so.s));
        HIP_OK(hipMemcpyFromSymbol(cold0, HIP_SYMBOL(owdev::g_trem_row_cold), sizeof cold0));
        Event e0, e1;
        e0.create(hipEventDefault); e1.create(hipEventDefault);
        HIP_OK(hipEventRecord(e0, so.s));
        for (long long t = 0; t < n; t += chunk) {
            const long long m = std::min(chunk, n - t);
            if (row) owdev::k_trem_traj_extend_row<<<dim3(1), dim3(64), 0, so.s>>>(dk.as<OwConsts>(), dstate.as<double>(), dr.as<double>() + t, t, m, dck.as<double>(), dbe.as<unsigned long long>());
            else owdev::k_trem_traj_extend<<<dim3(1), dim3(64), 0, so.s>>>(dk.as<OwConsts>(), dstate.as<double>(), dr.as<double>() + t, t, m, dck.as<double>(), dbe.as<unsigned long long>());
        }
        HIP_OK(hipEventRecord(e1, so.s));
        HIP_OK(hipGetLastError());
        HIP_OK(hipStreamSynchronize(so.s));
        float ms = 0.0f;
        HIP_OK(hipEventElapsedTime(&ms, e0, e1));
        if (ms_out) *ms_out = ms;
        HIP_OK(hipMemcpyFromSymbol(cold1, HIP_SYMBOL(owdev::g_trem_row_cold), sizeof cold1));
        if (cold_out) { cold_out[0] = cold1[0] - cold0[0]; cold_out[1] = cold1[1] - cold0[1]; }     // (of the trajectory launches; another store extending meanwhile would add its own)
        HIP_OK(hipMemcpy(r_out, dr.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(state_out, dstate.p, sizeof(double) * 18, hipMemcpyDeviceToHost));
        if (ckpt_out) HIP_OK(hipMemcpy(ckpt_out, dck.p, sizeof(double) * nck, hipMemcpyDeviceToHost));
        if (be_out) HIP_OK(hipMemcpy(be_out, dbe.p, sizeof(unsigned long long) * (1 + OW_TRAJ_BE_CAP), hipMemcpyDeviceToHost));
        return 0;
    } catch (const std::exception& ex) { (void)hipGetLastError(); set_err(std::string("ow_debug_trem_trajectory: ") + ex.what()); return -1; }
}
// Which literal-rebuild fast paths the host found usable for the melange preamp at chain rate `rate` (no device): bit 0 = the
// R-independent leading block could be replayed (ml_ok), bit 1 = the factors have the sparsity pattern ow_melange_col.h compiles in.
int ow_test_host_melange_paths(double rate) {
    try {
        std::unique_ptr<OwConsts> c(new OwConsts());
        owhip::build_consts(*c, rate < 88200.0 ? rate * 0.5 : rate, OW_PREAMP_MELANGE12);
        if (c->os_sr != rate) throw std::runtime_error("rate is not reachable as a chain rate");
        return (c->ml_ok ? 1 : 0) | (c->ml_sparse_ok ? 2 : 0);
    } catch (const std::exception& ex) { set_err(std::string("ow_test_host_melange_paths: ") + ex.what()); return -1; }
}
// The k-th acquisition (0-based) this thread makes from now on through the owning types of host_base.inc throws instead of calling HIP,
// then the hook disarms itself; k < 0 disarms it.  ow_test_live_resources: what is owned through those types right now, process-wide.
void ow_test_fail_acquire_after(int k) { g_fail_acquire_after = k < 0 ? -1 : k; }
uint64_t ow_test_live_resources(void) { return g_live_resources.load(std::memory_order_relaxed); }
void ow_test_inject_render_faults(ow_pool* p, int n_renders) { if (p) p->inject_faults = n_renders > 0 ? n_renders : 0; }
// One latched switch of a live pool (struct Switches; the OW_* environment variables are only read when a pool is created).
int ow_test_pool_set_switch(ow_pool* p, const char* name, int value) {
    if (!p || !name) return -1;
    const std::string n(name);
    if (hipSetDevice(p->device) != hipSuccess) return -1;
    invalidate_spec(p);                                   // a pending block-ahead result was produced under the old schedule
    if (hipStreamSynchronize(p->stream) != hipSuccess) return -1;
    if (!p->sw.set(name, value)) return -1;               // (trem_traj / trem_cache shape the pool at creation: environment only)
    if (n == "voice_attack" || n == "force_general") p->lists_valid = false;
    return 0;
}
int ow_test_pool_get_switch(const ow_pool* p, const char* name) {
    if (!p || !name) return -2;
    const std::string n(name);
    // read-only pseudo-names first: what the pool is doing, not what a switch says
    if (n == "voice_skew_active") return p->skew_next ? 1 : 0;   // the next steady launch takes the skewed variant
    if (n == "trem_traj") return p->traj ? 1 : 0;
    if (n == "blocks_steady") return (int)p->vl_steady.n_blocks;   // wavefront blocks of the voice lists the last render launched
    if (n == "blocks_general") return (int)p->vl_general.n_blocks;
    if (n == "blocks_attack") return (int)p->vl_attack.n_blocks;
    if (n == "blocks_steal") return (int)p->vl_steal.n_blocks;
    if (n == "midi_device_bursts") return (int)std::min<uint64_t>(p->vm_bursts, 0x7FFFFFFF);
    int v = 0;
    return p->sw.get(name, &v) ? v : -2;
}
// Which chain and output-stage kernels a block of such a pool gets (choose_chain / choose_post, host_pool.inc): host only, no pool.
int ow_test_block_plan(int preamp_kind, int power_amp_kind, int oversample, int ml_sparse_ok, int n_engines, int block_len, int to_pinned_block,
                       const char* switches, char* out, size_t cap) {
    if (!out) return -1;
    Switches sw;                                           // the defaults, not the environment
    for (const char* s = switches; s && *s;) {             // "name=value,name=value"
        const char* eq = std::strchr(s, '=');
        if (!eq) return -1;
        char* end = nullptr;
        const long v = std::strtol(eq + 1, &end, 10);
        if (end == eq + 1 || (*end && *end != ',')) return -1;
        if (!sw.set(std::string(s, eq).c_str(), (int)v)) return -1;
        s = *end ? end + 1 : end;
    }
    const ChainKernel chain = choose_chain(sw, preamp_kind, power_amp_kind, oversample != 0, ml_sparse_ok != 0, n_engines, block_len, to_pinned_block != 0);
    const PostKernel post = choose_post(sw, power_amp_kind, oversample != 0, n_engines, chain);
    const std::string plan = std::string(CHAIN_KERNEL_NAME[chain]) + (post != POST_NONE ? " + " : "") + POST_KERNEL_NAME[post];
    if (plan.size() + 1 > cap) return -1;
    std::memcpy(out, plan.c_str(), plan.size() + 1);
    return 0;
}
// Engines of the pool that read the shared trajectory / samples the store of the pool's rate holds (produced or enqueued) / its capacity.
int ow_test_pool_trajectory_info(const ow_pool* p, uint64_t out[3]) {
    if (!p || !out) return -1;
    out[0] = p->traj ? p->n_on_traj : 0; out[1] = 0; out[2] = 0;
    if (p->traj) { std::lock_guard<std::mutex> lk(p->traj->mu); out[1] = p->traj->len; out[2] = p->traj->cap_max; }
    return 0;
}
// The store behind the pool, in samples: [0] produced or enqueued, [1] known complete (finished launches), [2] what its buffers hold now,
// [3] its configured capacity, [4] t of the pool's oldest engine on it (what the next block needs is [4] + its chain-rate samples).
int ow_test_pool_trajectory_state(const ow_pool* p, uint64_t out[5]) {
    if (!p || !out) return -1;
    for (int i = 0; i < 5; ++i) out[i] = 0;
    if (!p->traj) return 0;
    std::lock_guard<std::mutex> lk(p->traj->mu);
    p->traj->in_flight();                                  // looks at the marks: refreshes `done`
    out[0] = p->traj->len; out[1] = p->traj->done; out[2] = p->traj->cap; out[3] = p->traj->cap_max;
    out[4] = (uint64_t)std::max<long long>(p->trem_clock - p->min_birth, 0);
    return 0;
}

// ---- diagnostics ---------------------------------------------------------------------------------
}  // extern "C"
namespace {
// One diagnostic run: the host arrays `in` copied into device buffers of their own (a null array: the buffer alone), the outputs `out`
// zeroed on the device, launch(inputs, outputs), the launch checked, the outputs copied back (a null array: workspace, left behind).
struct DebugIn { const void* host; size_t bytes; };
struct DebugOut { void* host; size_t bytes; };
template <class Launch> void debug_run(std::initializer_list<DebugIn> in, std::initializer_list<DebugOut> out, Launch launch) {
    std::vector<DevMem> di(in.size()), dout(out.size());
    size_t k = 0;
    for (const DebugIn& a : in) { di[k].alloc(a.bytes); if (a.host) HIP_OK(hipMemcpy(di[k].p, a.host, a.bytes, hipMemcpyHostToDevice)); ++k; }
    k = 0;
    for (const DebugOut& a : out) { dout[k].alloc(a.bytes); HIP_OK(hipMemset(dout[k].p, 0, a.bytes)); ++k; }
    launch(di.data(), dout.data());
    HIP_OK(hipGetLastError());
    k = 0;
    for (const DebugOut& a : out) { if (a.host) HIP_OK(hipMemcpy(a.host, dout[k].p, a.bytes, hipMemcpyDeviceToHost)); ++k; }
}
// A diagnostics hook's body under the hook's name: 0, or -1 with "<name>: <what went wrong>" as the library's last error.
template <class Body> int debug_hook(const char* name, Body body) {
    try { body(); return 0; } catch (const std::exception& ex) { (void)hipGetLastError(); set_err(std::string(name) + ": " + ex.what()); return -1; }
}
// The constants of the chain rate `rate`.  build_consts takes the HOST rate; a host rate >= 88.2 kHz runs the chain at that rate without
// oversampling (engine.rs:195)
std::unique_ptr<OwConsts> chain_rate_consts(double rate, int preamp_kind) {
    std::unique_ptr<OwConsts> hc(new OwConsts());
    owhip::build_consts(*hc, rate < 88200.0 ? rate * 0.5 : rate, preamp_kind);
    if (hc->os_sr != rate) throw std::runtime_error("rate is not reachable as a chain rate");
    return hc;
}
}  // namespace
extern "C" {
int ow_debug_mlp_raw(const uint8_t* notes, const double* velocities, size_t n, double* out, int use_mfma, int device) {
    return debug_hook("ow_debug_mlp_raw", [&] {
        if (!notes || !velocities || !out || n == 0) throw std::runtime_error("null argument");
        HIP_OK(hipSetDevice(device));
        debug_run({{notes, n}, {velocities, n * sizeof(double)}}, {{out, n * 11 * sizeof(double)}}, [&](const DevMem* i, const DevMem* o) {
            owdev::k_debug_mlp<<<dim3((unsigned)((n + 63) / 64)), dim3(64)>>>(i[0].as<uint8_t>(), i[1].as<double>(), (int)n, o[0].as<double>(), use_mfma);
        });
    });
}

int ow_debug_div(const double* a, const double* b, size_t n, double* fast, double* ieee, int device) {
    return debug_hook("ow_debug_div", [&] {
        if (!a || !b || !fast || !ieee) throw std::runtime_error("null argument");
        if (n == 0) return;
        HIP_OK(hipSetDevice(device));
        const size_t d = n * sizeof(double);
        debug_run({{a, d}, {b, d}}, {{fast, d}, {ieee, d}}, [&](const DevMem* i, const DevMem* o) {
            owdev::k_debug_div<<<dim3((unsigned)((n + 255) / 256)), dim3(256)>>>(i[0].as<double>(), i[1].as<double>(), n, o[0].as<double>(), o[1].as<double>());
        });
    });
}

int ow_debug_div_const(int which, const double* a, size_t n, double* fast, double* ieee, uint64_t* mismatches, int device) {
    return debug_hook("ow_debug_div_const", [&] {
        if (which < 0 || which > 7) throw std::runtime_error("unknown constant");
        HIP_OK(hipSetDevice(device));
        if (!a) {
            if (!mismatches) throw std::runtime_error("null argument");
            if (which != 0 && which != 6) throw std::runtime_error("no exhaustive numerator set for this constant");
            unsigned long long h = 0;
            debug_run({}, {{&h, sizeof h}}, [&](const DevMem*, const DevMem* o) {
                owdev::k_debug_div_draw_all<<<dim3(4096), dim3(256)>>>(which, o[0].as<unsigned long long>());
            });
            *mismatches = h;
            return;
        }
        if (!fast || !ieee) throw std::runtime_error("null argument");
        if (n == 0) return;
        const size_t d = n * sizeof(double);
        debug_run({{a, d}}, {{fast, d}, {ieee, d}}, [&](const DevMem* i, const DevMem* o) {
            owdev::k_debug_div_const<<<dim3((unsigned)((n + 255) / 256)), dim3(256)>>>(which, i[0].as<double>(), n, o[0].as<double>(), o[1].as<double>());
        });
    });
}

int ow_debug_div_forms(int mode, const double* a, const double* b, const double* y, size_t n, double* fast, double* ieee, int device) {
    return debug_hook("ow_debug_div_forms", [&] {
        if (!a || !b || !fast || !ieee || mode < 0 || mode > 2 || (mode == 0 && !y)) throw std::runtime_error("bad argument");
        if (n == 0) return;
        HIP_OK(hipSetDevice(device));
        const size_t d = n * sizeof(double);
        debug_run({{a, d}, {b, d}, {y, d}}, {{fast, d}, {ieee, d}}, [&](const DevMem* i, const DevMem* o) {
            owdev::k_debug_div_forms<<<dim3((unsigned)((n + 255) / 256)), dim3(256)>>>(mode, i[0].as<double>(), i[1].as<double>(), i[2].as<double>(), n, o[0].as<double>(), o[1].as<double>());
        });
    });
}

int ow_debug_unary(int which, const double* x, size_t n, double* fast, double* lib, int device) {
    return debug_hook("ow_debug_unary", [&] {
        if (!x || !fast || !lib || which < 0 || which > 6) throw std::runtime_error("null argument or unknown function");
        if (n == 0) return;
        HIP_OK(hipSetDevice(device));
        const size_t d = n * sizeof(double);
        debug_run({{x, d}}, {{fast, d}, {lib, d}}, [&](const DevMem* i, const DevMem* o) {
            owdev::k_debug_exp<<<dim3((unsigned)((n + 255) / 256)), dim3(256)>>>(which, i[0].as<double>(), n, o[0].as<double>(), o[1].as<double>());
        });
    });
}

int ow_debug_dk_step(int form, double rate, const double* states_in, const double* input, const double* g_ldr, const double* g_ldr_prev, size_t n,
                     double* states_out, double* out, int device) {
    return debug_hook("ow_debug_dk_step", [&] {
        if (!states_in || !input || !g_ldr || !g_ldr_prev || !states_out || !out || form < 0 || form > 3 || !(rate > 0.0)) throw std::runtime_error("bad argument");
        if (n == 0) return;
        if (n > (size_t)1 << 24) throw std::runtime_error("too many cases");
        HIP_OK(hipSetDevice(device));
        const std::unique_ptr<OwConsts> hc = chain_rate_consts(rate, OW_PREAMP_LEGACY8);
        std::vector<double> rows(14 * n);                      // the chain kernels' state rows: [field][case]
        for (size_t c = 0; c < n; ++c)
            for (int f = 0; f < 14; ++f) rows[(size_t)f * n + c] = states_in[c * 14 + f];
        const size_t d = sizeof(double) * n;
        const size_t per_wave[4] = {64, 128, 16, 4};            // cases of one wavefront: lane | lane = (main, shadow) | quad | row of sixteen
        const dim3 grid((unsigned)((n + per_wave[form] - 1) / per_wave[form])), block(64);
        debug_run({{hc.get(), sizeof(OwConsts)}, {rows.data(), 14 * d}, {input, d}, {g_ldr, d}, {g_ldr_prev, d}}, {{rows.data(), 14 * d}, {out, d}},
                  [&](const DevMem* i, const DevMem* o) {
            const OwConsts* K = i[0].as<OwConsts>();
            const DevMem &dIn = i[1], &dX = i[2], &dG = i[3], &dGp = i[4], &dOut = o[0], &dO = o[1];
            switch (form) {
                case 0: owdev::k_debug_dk_step<owdev::DKF_LANE><<<grid, block>>>(K, dIn.as<double>(), dX.as<double>(), dG.as<double>(), dGp.as<double>(), (int)n, dOut.as<double>(), dO.as<double>()); break;
                case 1: owdev::k_debug_dk_step<owdev::DKF_PAIR><<<grid, block>>>(K, dIn.as<double>(), dX.as<double>(), dG.as<double>(), dGp.as<double>(), (int)n, dOut.as<double>(), dO.as<double>()); break;
                case 2: owdev::k_debug_dk_step<owdev::DKF_WIDE><<<grid, block>>>(K, dIn.as<double>(), dX.as<double>(), dG.as<double>(), dGp.as<double>(), (int)n, dOut.as<double>(), dO.as<double>()); break;
                default: owdev::k_debug_dk_step<owdev::DKF_ROW><<<grid, block>>>(K, dIn.as<double>(), dX.as<double>(), dG.as<double>(), dGp.as<double>(), (int)n, dOut.as<double>(), dO.as<double>()); break;
            }
        });
        for (size_t c = 0; c < n; ++c)
            for (int f = 0; f < 14; ++f) states_out[c * 14 + f] = rows[(size_t)f * n + c];
    });
}

int ow_debug_trem_step(int form, double rate, const double* states_in, size_t n, double* states_out, double* out, unsigned long long* info, int device) {
    return debug_hook("ow_debug_trem_step", [&] {
        if (!states_in || !states_out || !out || !info || form < 0 || form > 2 || !(rate > 0.0)) throw std::runtime_error("bad argument");
        if (n == 0) return;
        if (n > (size_t)1 << 22) throw std::runtime_error("too many cases");
        HIP_OK(hipSetDevice(device));
        const std::unique_ptr<OwConsts> hc = chain_rate_consts(rate, OW_PREAMP_LEGACY8);
        // the eighteen tremolo rows: [field][case] for the lane and quad forms, [case][field] for the row form; cell at rest, counter 0
        const bool by_case = form == 2;
        auto at = [&](size_t f, size_t c) { return by_case ? c * 18 + f : f * n + c; };
        std::vector<double> rows(18 * n, 0.0);
        for (size_t c = 0; c < n; ++c) {
            for (size_t f = 0; f < 15; ++f) rows[at(f, c)] = states_in[c * 15 + f];
            rows[at(CS_T_RLDR, c)] = 1000000.0;
        }
        const size_t per_wave[3] = {64, 16, 1};                  // cases of one wavefront: lane | quad | the whole wavefront
        const dim3 grid((unsigned)((n + per_wave[form] - 1) / per_wave[form])), block(64);
        debug_run({{hc.get(), sizeof(OwConsts)}, {rows.data(), sizeof(double) * 18 * n}},
                  {{rows.data(), sizeof(double) * 18 * n}, {out, sizeof(double) * n}, {info, sizeof(unsigned long long) * n}}, [&](const DevMem* i, const DevMem* o) {
            const OwConsts* K = i[0].as<OwConsts>();
            const DevMem &dIn = i[1], &dOut = o[0], &dO = o[1], &dI = o[2];
            switch (form) {
                case 0: owdev::k_debug_trem_step<owdev::TSF_LANE><<<grid, block>>>(K, dIn.as<double>(), (int)n, dOut.as<double>(), dO.as<double>(), dI.as<unsigned long long>()); break;
                case 1: owdev::k_debug_trem_step<owdev::TSF_WIDE><<<grid, block>>>(K, dIn.as<double>(), (int)n, dOut.as<double>(), dO.as<double>(), dI.as<unsigned long long>()); break;
                default: owdev::k_debug_trem_step<owdev::TSF_ROW><<<grid, block>>>(K, dIn.as<double>(), (int)n, dOut.as<double>(), dO.as<double>(), dI.as<unsigned long long>()); break;
            }
        });
        for (size_t c = 0; c < n; ++c)
            for (size_t f = 0; f < 15; ++f) states_out[c * 15 + f] = rows[at(f, c)];
    });
}
int ow_debug_mel_step(int form, double rate, const double* states_in, const double* input, const double* r_ldr, size_t n, double* states_out, double* out,
                      unsigned* info, int device) {
    return debug_hook("ow_debug_mel_step", [&] {
        if (!states_in || !input || !r_ldr || !states_out || !out || !info || form < 0 || form > 6 || !(rate > 0.0)) throw std::runtime_error("bad argument");
        if (n == 0) return;
        if (n > (size_t)1 << 22) throw std::runtime_error("too many cases");
        HIP_OK(hipSetDevice(device));
        const std::unique_ptr<OwConsts> hc = chain_rate_consts(rate, OW_PREAMP_MELANGE12);
        // the pool launches a form only where the host found its fast path usable (host_pool.inc)
        if (form == 1 && !hc->ml_ok) throw std::runtime_error("the leading block cannot be replayed at this rate");
        if (form >= 3 && !hc->ml_sparse_ok) throw std::runtime_error("the factors do not have the compiled-in pattern at this rate");
        const size_t pairs = (n + 1) / 2;
        const size_t per_block = form == 0 ? 64 : (form <= 4 ? 32 : 64);          // cases | pairs | pairs | engines of one wavefront
        const size_t units = form == 0 ? n : pairs;
        const size_t blocks = (units + per_block - 1) / per_block;
        // the generic rebuilds' workspace, as pool_create sizes d_mel_lu: lane-minor columns with 32 spare pairs for lanes without an
        // engine (col / eng), one [12][12][32] slab per workgroup (lit)
        const size_t lu_ld = 2 * (pairs + 32);
        const size_t lu_doubles = 144 * std::max<size_t>(lu_ld, 32 * (blocks + 1));
        const size_t d = sizeof(double) * n;
        const dim3 grid((unsigned)blocks), block(64);
        debug_run({{hc.get(), sizeof(OwConsts)}, {states_in, 21 * d}, {input, d}, {r_ldr, d}},
                  {{states_out, 21 * d}, {out, d}, {info, sizeof(unsigned) * 2 * n}, {nullptr, sizeof(double) * lu_doubles}}, [&](const DevMem* i, const DevMem* o) {
            const OwConsts* K = i[0].as<OwConsts>();
            const DevMem &dS = i[1], &dX = i[2], &dR = i[3], &dSo = o[0], &dO = o[1], &dI = o[2], &dLu = o[3];
#define OW_MEL_STEP_LAUNCH(F) owdev::k_debug_mel_step<F><<<grid, block>>>(K, dS.as<double>(), dX.as<double>(), dR.as<double>(), (int)n, dSo.as<double>(), \
                                                                         dO.as<double>(), dI.as<unsigned>(), dLu.as<double>(), lu_ld)
            switch (form) {
                case 0: OW_MEL_STEP_LAUNCH(owdev::MSF_RANK1); break;
                case 1: OW_MEL_STEP_LAUNCH(owdev::MSF_LIT_FAST); break;
                case 2: OW_MEL_STEP_LAUNCH(owdev::MSF_LIT_GENERIC); break;
                case 3: OW_MEL_STEP_LAUNCH(owdev::MSF_COL_FAST); break;
                case 4: OW_MEL_STEP_LAUNCH(owdev::MSF_COL_GENERIC); break;
                case 5: OW_MEL_STEP_LAUNCH(owdev::MSF_ENG_FAST); break;
                default: OW_MEL_STEP_LAUNCH(owdev::MSF_ENG_GENERIC); break;
            }
#undef OW_MEL_STEP_LAUNCH
        });
    });
}
}  // extern "C"
