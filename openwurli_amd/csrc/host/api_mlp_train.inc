// openwurli-hip host side, part of openwurli_hip.hip (one translation unit): C-ABI: training note-on MLP weight sets on the device
// (ml/train_mlp.py's train(), many models per call).  The host validates, hands each model the lists of its train and validation rows
// and its loss denominators, and launches k_mlp_train (ow_mlp_train.h) once: grid = models, one wavefront each.
static_assert(sizeof(ow_mlp_train_result) == sizeof(owdev::MlpTrainResultDev), "ow_mlp_train_result is written by the device as MlpTrainResultDev");
static_assert(offsetof(ow_mlp_weights, target_means) == sizeof(double) * owdev::MT_PARAMS, "the 507 parameters lead ow_mlp_weights");
static_assert(offsetof(ow_mlp_weights, b1) == 8 * owdev::MT_B1 && offsetof(ow_mlp_weights, w2) == 8 * owdev::MT_W2 && offsetof(ow_mlp_weights, b2) == 8 * owdev::MT_B2 &&
              offsetof(ow_mlp_weights, w3) == 8 * owdev::MT_W3 && offsetof(ow_mlp_weights, b3) == 8 * owdev::MT_B3, "k_mlp_train's offsets are ow_mlp_weights'");
namespace {
namespace mlp_train {

void check_model(const std::string& at, const ow_mlp_train_model& m, uint32_t n_rows) {
    check_positive_finite(at, "lr", m.lr);
    check_positive_finite(at, "huber_delta", m.huber_delta);
    if (!(std::isfinite(m.min_lr) && m.min_lr >= 0.0)) throw std::runtime_error(at + "min_lr is not a finite non-negative number");
    if (!(std::isfinite(m.weight_decay) && m.weight_decay >= 0.0)) throw std::runtime_error(at + "weight_decay is not a finite non-negative number");
    if (!(m.sched_factor > 0.0 && m.sched_factor < 1.0)) throw std::runtime_error(at + "sched_factor is not inside (0, 1)");
    if (m.epochs == 0) throw std::runtime_error(at + "epochs is 0");
    if ((uint64_t)n_rows * m.epochs > (uint64_t)OW_MLP_TRAIN_MAX_ROW_EPOCHS)
        throw std::runtime_error(at + "n_rows x epochs = " + std::to_string((uint64_t)n_rows * m.epochs) + " is above " + std::to_string(OW_MLP_TRAIN_MAX_ROW_EPOCHS) +
                                 " (OW_MLP_TRAIN_MAX_ROW_EPOCHS: a model is one serial wavefront)");
}

}  // namespace mlp_train
}  // namespace

extern "C" {

int ow_mlp_train(const double* inputs, const double* targets, const uint8_t* mask, const double* row_weights, const uint8_t* split,
                 const ow_mlp_weights* init, const ow_mlp_train_model* models, size_t n_models, const ow_mlp_train_cfg* cfg,
                 ow_mlp_weights* best_out, ow_mlp_train_result* results, double* history_out) {
    try {
        if (!cfg) throw std::runtime_error("null argument");
        if (cfg->struct_size != sizeof(ow_mlp_train_cfg) || cfg->model_size != sizeof(ow_mlp_train_model))
            throw std::runtime_error(abi_mismatch("ow_mlp_train_cfg.struct_size / model_size do"));
        if (!inputs || !targets || !mask || !row_weights || !split || !init || !models || !best_out || !results) throw std::runtime_error("null argument");
        const size_t n = cfg->n_rows;
        if (n == 0) throw std::runtime_error("n_rows is 0");
        if (n_models == 0) return 0;
        if (n_models > MLP_MAX_SETS) throw std::runtime_error("more than 65535 models in one call");
        // each model owns a list of its train rows and one of its validation rows: at most 2 x n_rows indices, 2^28 (1 GiB) for the call
        if (n_models * n > ((size_t)1 << 27)) throw std::runtime_error("n_models x n_rows is above 2^27 (the models' row lists would pass 1 GiB)");
        if (history_out && n_models * (size_t)cfg->history_epochs > ((size_t)1 << 27)) throw std::runtime_error("n_models x history_epochs is above 2^27 (history_out would pass 3 GiB)");
        std::vector<uint32_t> mask_bits(n, 0u);
        for (size_t r = 0; r < n; ++r) {
            const std::string at = "row " + std::to_string(r) + ": ";
            for (int c = 0; c < 2; ++c) check_finite(at, ("inputs[" + std::to_string(c) + "]").c_str(), inputs[2 * r + c]);
            for (int k = 0; k < 11; ++k) {
                check_finite(at, ("targets[" + std::to_string(k) + "]").c_str(), targets[11 * r + k]);
                if (mask[11 * r + k]) mask_bits[r] |= 1u << k;
            }
            check_finite(at, "row_weights", row_weights[r]);
        }
        check_weight_sets(init, n_models, "model ", "init.");
        std::vector<owdev::MlpTrainModelDev> dev(n_models);
        std::vector<uint32_t> rows;
        for (size_t i = 0; i < n_models; ++i) {
            const std::string at = "model " + std::to_string(i) + ": ";
            const ow_mlp_train_model& m = models[i];
            mlp_train::check_model(at, m, cfg->n_rows);
            if (history_out && cfg->history_epochs < m.epochs)
                throw std::runtime_error(at + "epochs " + std::to_string(m.epochs) + " is above history_epochs " + std::to_string(cfg->history_epochs));
            owdev::MlpTrainModelDev& d = dev[i];
            d.lr = m.lr; d.min_lr = m.min_lr; d.weight_decay = m.weight_decay; d.huber_delta = m.huber_delta; d.sched_factor = m.sched_factor;
            d.epochs = m.epochs; d.patience = m.patience; d.sched_patience = m.sched_patience; d.target_mask = m.target_mask & 0x7FFu;
            d.rows_at = rows.size();
            const uint8_t* sp = split + i * n;
            uint64_t nv[2] = {0, 0};
            uint32_t cnt[2] = {0, 0};
            for (int part = 0; part < 2; ++part)               // the train rows, then the validation rows, each in the data's order
                for (size_t r = 0; r < n; ++r)
                    if (sp[r] >> part & 1) {
                        rows.push_back((uint32_t)r);
                        cnt[part] += 1;
                        nv[part] += (uint64_t)__builtin_popcount(mask_bits[r] & d.target_mask);
                    }
            // the reference would divide by zero (train) or watch a constant 0 (validation)
            if (nv[0] == 0) throw std::runtime_error(at + "split / target_mask leave no masked-in entry among the train rows");
            if (nv[1] == 0) throw std::runtime_error(at + "split / target_mask leave no masked-in entry among the validation rows");
            d.n_train = cnt[0]; d.n_val = cnt[1];
            d.n_valid_train = (double)nv[0]; d.n_valid_val = (double)nv[1];
        }
        require_device(cfg->device);
        StreamOwner so;
        so.create();
        hipStream_t st = so.s;
        DevMem m_in, m_tg, m_mb, m_rw, m_rows, m_models, m_best, m_res, m_hist;
        const size_t hist_bytes = history_out ? sizeof(double) * 3 * n_models * cfg->history_epochs : 0;
        m_in.alloc(sizeof(double) * 2 * n); m_tg.alloc(sizeof(double) * 11 * n); m_mb.alloc(sizeof(uint32_t) * n); m_rw.alloc(sizeof(double) * n);
        m_rows.alloc(sizeof(uint32_t) * rows.size()); m_models.alloc(sizeof(owdev::MlpTrainModelDev) * n_models);
        m_best.alloc(sizeof(ow_mlp_weights) * n_models); m_res.alloc(sizeof(ow_mlp_train_result) * n_models);
        if (hist_bytes) m_hist.alloc(hist_bytes);
        HIP_OK(hipMemcpyAsync(m_in.p, inputs, sizeof(double) * 2 * n, hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(m_tg.p, targets, sizeof(double) * 11 * n, hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(m_mb.p, mask_bits.data(), sizeof(uint32_t) * n, hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(m_rw.p, row_weights, sizeof(double) * n, hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(m_rows.p, rows.data(), sizeof(uint32_t) * rows.size(), hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(m_models.p, dev.data(), sizeof(owdev::MlpTrainModelDev) * n_models, hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(m_best.p, init, sizeof(ow_mlp_weights) * n_models, hipMemcpyHostToDevice, st));      // the best state starts as the initial set
        if (hist_bytes) HIP_OK(hipMemsetAsync(m_hist.p, 0, hist_bytes, st));
        Event ev0, ev1;
        if (cfg->kernel_ms_out) { ev0.create(hipEventDefault); ev1.create(hipEventDefault); HIP_OK(hipEventRecord(ev0.e, st)); }
        const owdev::MlpTrainData data{m_in.as<double>(), m_tg.as<double>(), m_mb.as<uint32_t>(), m_rw.as<double>()};
        owdev::k_mlp_train<<<dim3((unsigned)n_models), dim3(64), 0, st>>>(data, m_rows.as<uint32_t>(), m_models.as<owdev::MlpTrainModelDev>(),
                                                                         m_best.as<owdev::MlpWeightsDev>(), m_res.as<owdev::MlpTrainResultDev>(),
                                                                         hist_bytes ? m_hist.as<double>() : nullptr, cfg->history_epochs);
        HIP_OK(hipGetLastError());
        if (cfg->kernel_ms_out) HIP_OK(hipEventRecord(ev1.e, st));
        HIP_OK(hipMemcpyAsync(best_out, m_best.p, sizeof(ow_mlp_weights) * n_models, hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(results, m_res.p, sizeof(ow_mlp_train_result) * n_models, hipMemcpyDeviceToHost, st));
        if (hist_bytes) HIP_OK(hipMemcpyAsync(history_out, m_hist.p, hist_bytes, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        if (cfg->kernel_ms_out) {
            float ms = 0.0f;
            HIP_OK(hipEventElapsedTime(&ms, ev0.e, ev1.e));
            *cfg->kernel_ms_out = (double)ms;
        }
        return 0;
    } catch (const std::exception& ex) { set_err(std::string("ow_mlp_train: ") + ex.what()); return -1; }
}

}  // extern "C"
