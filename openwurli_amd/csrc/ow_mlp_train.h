// openwurli-hip: training of the note-on MLP (2 -> 16 -> 16 -> 11; ml/train_mlp.py's train()) -- one wavefront trains one model, the
// whole run inside one launch: every epoch's forward and backward pass over the train rows, Adam, the validation pass,
// ReduceLROnPlateau, early stopping and the best-state snapshot.  All arithmetic is f64.
//
//   Rows are walked in tiles of 64 (lane = row), four 16-row MFMA tiles.  Layer 1 (K = 2) is two multiply-adds per hidden unit; layers
//   2 and 3 run on v_mfma_f64_16x16x4_f64 exactly as mlp_layer_mfma does (A = weights, B = activations of 16 rows, bias as C).  The
//   backward pass has the same shapes:
//     dW3 = dY^T . H2, dW2 = dZ2^T . H1   K = the row index: A[i][k] = dY[row k][unit i], B[k][j] = H[row k][unit j]; ONE accumulator per
//                                         matrix is carried across all row tiles of the epoch, so no cross-lane reduction is needed;
//     dH2 = dY . W3,   dH1 = dZ2 . W2     the transposed-weight products: A[i][k] = W[k][i], B as in the forward pass.
//   Bias and layer-1 gradients: lane (unit j = lane & 15, quarter q = lane >> 4) sums the 16 rows of its quarter from the LDS tile, the four
//   quarters meet at the end of the epoch.  Every sum has a fixed order (no atomics): two calls give the same bits, and a model's result
//   does not depend on its neighbours in the grid.
//
//   State: the 507 parameters and their gradients in LDS, Adam's moments in registers (8 per lane each), the best state in global memory
//   (best_out itself, which the host has filled with the initial set).  Rows outside the model's split never enter: the host hands each
//   model the list of its train rows and of its validation rows; lanes past the end of a list carry zero inputs, mask and weight, so they
//   contribute exact zeros (a factor 0.0 on a finite term: with diverged weights 0 x inf is NaN, as in torch; such a lane reads row 0's
//   targets, which is valid memory).
//
// Fragment layout as in ow_mlp_mfma.h: A: lane l holds A[i = l & 15][k = l >> 4]; B: B[k = l >> 4][j = l & 15];
// C/D: lane l, register r holds D[row = (l >> 4) + 4 r][col = l & 15].
#pragma once
#include "ow_mlp_mfma.h"

namespace owdev {

// one model of a call, as the host prepares it
struct MlpTrainModelDev {
    double lr, min_lr, weight_decay, huber_delta, sched_factor;
    double n_valid_train, n_valid_val;      // masked-in entries of the train / validation rows (the loss denominators)
    uint32_t epochs, patience, sched_patience, target_mask;
    uint32_t n_train, n_val;                // rows[rows_at .. +n_train) are the train rows, the n_val validation rows follow
    uint64_t rows_at;
};
// ow_mlp_train_result (include/openwurli_hip.h)
struct MlpTrainResultDev {
    double best_val_loss, last_train_loss, last_val_loss, last_lr;
    uint32_t best_epoch, epochs_run, lr_reductions, status;
};

constexpr int MT_W1 = 0, MT_B1 = 32, MT_W2 = 48, MT_B2 = 304, MT_W3 = 320, MT_B3 = 496, MT_PARAMS = 507;    // offsets in ow_mlp_weights, in doubles
constexpr int MT_LD = 17;                   // a tile row: 16 units, padded

// the data all models share, read-only
struct MlpTrainData {
    const double* inputs;       // [n_rows][2]
    const double* targets;      // [n_rows][11], standardised
    const uint32_t* mask_bits;  // [n_rows]: bit k = target k of the row is valid
    const double* row_weights;  // [n_rows]
};

__device__ inline double mt_uniform(double x) {        // the first lane's value as a scalar: every lane holds the same bits already
    const unsigned long long u = (unsigned long long)__double_as_longlong(x);
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)u), hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(u >> 32));
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
// sum over the wavefront, the same bits in every lane (a + b == b + a at every step of the butterfly)
__device__ inline double mt_wave_sum(double x) {
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) x += __shfl_xor(x, s, 64);
    return mt_uniform(x);
}

// beta^t for a step count t >= 1 by squaring: at most a few ulp of beta^t from the library's pow, i.e. below 1e-16 of the bias
// correction 1 - beta^t it enters
__device__ inline double mt_powi(double beta, uint32_t t) {
    double r = 1.0;
    for (; t; t >>= 1, beta *= beta)
        if (t & 1u) r *= beta;
    return r;
}

// the weights as MFMA A operands and the biases as C operands, refreshed after every Adam step
struct MtFrags {
    double w2f[4], w3f[4];      // forward:  A[i][k] = W[i][4c + k]
    double w2t[4], w3t[3];      // backward: A[i][k] = W[4c + k][i]
    v4f64 b2, b3;
};
__device__ inline void mt_load_frags(const double* __restrict__ P, MtFrags& f) {
    const int lane = threadIdx.x & 63, i = lane & 15, kq = lane >> 4;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        f.w2f[c] = P[MT_W2 + i * 16 + 4 * c + kq];
        f.w3f[c] = i < 11 ? P[MT_W3 + i * 16 + 4 * c + kq] : 0.0;
        f.w2t[c] = P[MT_W2 + (4 * c + kq) * 16 + i];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) f.w3t[c] = 4 * c + kq < 11 ? P[MT_W3 + (4 * c + kq) * 16 + i] : 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        f.b2[r] = P[MT_B2 + kq + 4 * r];
        f.b3[r] = kq + 4 * r < 11 ? P[MT_B3 + kq + 4 * r] : 0.0;
    }
}

// One row per lane of a tile: what the loss needs of it.  Lanes past the end of the list: zero inputs, empty mask, zero weight.
struct MtRow { double x0, x1, w; uint32_t mask; size_t at; };
__device__ inline MtRow mt_fetch_row(const MlpTrainData& d, const uint32_t* __restrict__ rows, uint32_t first, uint32_t count, uint32_t target_mask) {
    const uint32_t q = first + (threadIdx.x & 63);
    MtRow r;
    if (q < count) {
        r.at = rows[q];
        r.x0 = d.inputs[2 * r.at]; r.x1 = d.inputs[2 * r.at + 1];
        r.w = d.row_weights[r.at];
        r.mask = d.mask_bits[r.at] & target_mask;
    } else { r.at = 0; r.x0 = r.x1 = r.w = 0.0; r.mask = 0u; }
    return r;
}

// Forward pass of one tile: ta <- H1 (after ReLU), tb <- H2 (after ReLU), tc <- Y (columns 11..15 are 0.0).  xs <- the inputs.
// Ends behind a barrier.
__device__ inline void mt_forward(const double* __restrict__ P, const MtFrags& f, const MtRow& row, double* __restrict__ ta, double* __restrict__ tb,
                                  double* __restrict__ tc, double* __restrict__ xs) {
    const int lane = threadIdx.x & 63, i = lane & 15, kq = lane >> 4;
    xs[2 * lane] = row.x0; xs[2 * lane + 1] = row.x1;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        double z = P[MT_B1 + j];
        z += P[MT_W1 + 2 * j] * row.x0;
        z += P[MT_W1 + 2 * j + 1] * row.x1;
        ta[lane * MT_LD + j] = fmax(z, 0.0);
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        v4f64 acc = f.b2;
#pragma unroll
        for (int c = 0; c < 4; ++c) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(f.w2f[c], ta[(16 * t + i) * MT_LD + 4 * c + kq], acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) tb[(16 * t + i) * MT_LD + kq + 4 * r] = fmax(acc[r], 0.0);
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        v4f64 acc = f.b3;
#pragma unroll
        for (int c = 0; c < 4; ++c) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(f.w3f[c], tb[(16 * t + i) * MT_LD + 4 * c + kq], acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) tc[(16 * t + i) * MT_LD + kq + 4 * r] = acc[r];
    }
    __syncthreads();
}

// The lane's row of tc against its targets: returns the row's loss terms (mask x weight x Huber, summed) and, with GRAD, replaces the row
// of tc by dLoss/dY (grad_scale = 1 / n_valid).  No barrier.  Written without selects (each would hold a lane mask in a scalar pair
// across the unrolled loop); the same bits as the branches they stand for:
//   Huber:      c = min(|d|, delta); c (|d| - c / 2) is 0.5 d^2 for |d| < delta (a power-of-two factor moves freely) and delta (|d| - delta / 2) beyond;
//   derivative: clamp(d, -delta, delta) is d for |d| < delta and delta sign(d) beyond;
//   mask:       a factor 1.0 or 0.0 on the row's weight (a masked-out entry of a finite prediction is an exact zero).
template <bool GRAD>
__device__ inline double mt_loss_row(const MlpTrainData& d, const MtRow& row, double delta, double grad_scale, double* __restrict__ tc) {
    const int lane = threadIdx.x & 63;
    double sum = 0.0;
    const double gw = grad_scale * row.w;
#pragma unroll
    for (int k = 0; k < 11; ++k) {
        const double on = (double)((row.mask >> k) & 1u);
        const double diff = tc[lane * MT_LD + k] - d.targets[row.at * 11 + k];
        const double a = fabs(diff), c = fmin(a, delta);
        sum += (c * (a - 0.5 * c)) * (row.w * on);
        if (GRAD) tc[lane * MT_LD + k] = (gw * on) * fmax(fmin(diff, delta), -delta);
    }
    return sum;
}

// sum over the 16 rows of this lane's quarter of column (lane & 15) of a tile
__device__ inline double mt_quarter_sum(const double* __restrict__ tile) {
    const int lane = threadIdx.x & 63, j = lane & 15, q = lane >> 4;
    double s = 0.0;
#pragma unroll 4
    for (int r = 0; r < 16; ++r) s += tile[(16 * q + r) * MT_LD + j];
    return s;
}
// the four quarters of a per-lane partial sum, the same bits in the four lanes of a unit
__device__ inline double mt_quarters(double x) {
    x += __shfl_xor(x, 16, 64);
    x += __shfl_xor(x, 32, 64);
    return x;
}

// grid = models, block = one wavefront.  best_out[model] holds the initial set on entry (its target_means / target_stds stay as they are).
// history: nullptr or [n_models][history_epochs][3], zeroed by the host.
__global__ __launch_bounds__(64) void k_mlp_train(MlpTrainData data, const uint32_t* __restrict__ rows, const MlpTrainModelDev* __restrict__ models,
                                                  MlpWeightsDev* __restrict__ best_out, MlpTrainResultDev* __restrict__ results,
                                                  double* __restrict__ history, uint32_t history_epochs) {
    __shared__ double P[512];                    // the parameters, in ow_mlp_weights' order
    __shared__ double TA[64 * MT_LD], TB[64 * MT_LD], TC[64 * MT_LD], XS[128];
    double* const G = TA;                        // the epoch's gradient, written once the last tile is done with TA
    const int lane = threadIdx.x & 63, i = lane & 15, kq = lane >> 4;
    const MlpTrainModelDev& mo = models[blockIdx.x];      // read where it is used: scalar loads, not thirty live registers
    const uint32_t* const train_rows = rows + mo.rows_at;
    const uint32_t* const val_rows = train_rows + mo.n_train;
    double* const best = reinterpret_cast<double*>(best_out + blockIdx.x);

    double am[8], av[8];                         // Adam's moments of parameters lane + 64 k
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int p = lane + 64 * k;
        if (p < 512) P[p] = p < MT_PARAMS ? best[p] : 0.0;
        am[k] = av[k] = 0.0;
    }
    __syncthreads();
    MtFrags f;
    mt_load_frags(P, f);

    const double inv_nv_train = 1.0 / mo.n_valid_train;
    double lr = mo.lr, best_val = __builtin_inf(), sched_best = __builtin_inf();
    double train_loss = 0.0, val_loss = 0.0;
    uint32_t bad = 0, stale = 0, best_epoch = 0, reductions = 0, e = 0;

    for (;;) {
        // ---- forward and backward over the train rows
        v4f64 dw3 = {0.0, 0.0, 0.0, 0.0}, dw2 = {0.0, 0.0, 0.0, 0.0};
        double gb3 = 0.0, gb2 = 0.0, gb1 = 0.0, gw10 = 0.0, gw11 = 0.0, loss = 0.0;
        for (uint32_t first = 0; first < mo.n_train; first += 64) {
            const MtRow row = mt_fetch_row(data, train_rows, first, mo.n_train, mo.target_mask);
            mt_forward(P, f, row, TA, TB, TC, XS);
            loss += mt_loss_row<true>(data, row, mo.huber_delta, inv_nv_train, TC);
            __syncthreads();                     // TC = dY
#pragma unroll 4
            for (int c = 0; c < 16; ++c)         // dW3 += dY^T . H2, four rows per step
                dw3 = __builtin_amdgcn_mfma_f64_16x16x4f64(TC[(4 * c + kq) * MT_LD + i], TB[(4 * c + kq) * MT_LD + i], dw3, 0, 0, 0);
            gb3 += mt_quarter_sum(TC);
            double dz[4][4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {        // dH2 = dY . W3 (K = 11, padded to 12), through the ReLU of layer 2
                v4f64 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int c = 0; c < 3; ++c) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(f.w3t[c], TC[(16 * t + i) * MT_LD + 4 * c + kq], acc, 0, 0, 0);
#pragma unroll
                for (int r = 0; r < 4; ++r) dz[t][r] = TB[(16 * t + i) * MT_LD + kq + 4 * r] > 0.0 ? acc[r] : 0.0;
            }
            __syncthreads();                     // every read of dY is done
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) TC[(16 * t + i) * MT_LD + kq + 4 * r] = dz[t][r];
            __syncthreads();                     // TC = dZ2
#pragma unroll 4
            for (int c = 0; c < 16; ++c)         // dW2 += dZ2^T . H1
                dw2 = __builtin_amdgcn_mfma_f64_16x16x4f64(TC[(4 * c + kq) * MT_LD + i], TA[(4 * c + kq) * MT_LD + i], dw2, 0, 0, 0);
            gb2 += mt_quarter_sum(TC);
#pragma unroll
            for (int t = 0; t < 4; ++t) {        // dH1 = dZ2 . W2, through the ReLU of layer 1; H2 is no longer needed: TB = dZ1
                v4f64 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int c = 0; c < 4; ++c) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(f.w2t[c], TC[(16 * t + i) * MT_LD + 4 * c + kq], acc, 0, 0, 0);
#pragma unroll
                for (int r = 0; r < 4; ++r) TB[(16 * t + i) * MT_LD + kq + 4 * r] = TA[(16 * t + i) * MT_LD + kq + 4 * r] > 0.0 ? acc[r] : 0.0;
            }
            __syncthreads();                     // TB = dZ1
            {
                double s = 0.0, s0 = 0.0, s1 = 0.0;
#pragma unroll 4
                for (int r = 0; r < 16; ++r) {   // layer 1: db1 and dW1 = dZ1^T . X over the 16 rows of this lane's quarter
                    const int at = 16 * kq + r;
                    const double z = TB[at * MT_LD + i];
                    s += z;
                    s0 += z * XS[2 * at];
                    s1 += z * XS[2 * at + 1];
                }
                gb1 += s; gw10 += s0; gw11 += s1;
            }
            __syncthreads();                     // the next tile overwrites TA, TB, XS
        }
        train_loss = mt_wave_sum(loss) / mo.n_valid_train;

        // ---- the gradient, in the parameters' order
        gb3 = mt_quarters(gb3); gb2 = mt_quarters(gb2); gb1 = mt_quarters(gb1); gw10 = mt_quarters(gw10); gw11 = mt_quarters(gw11);
#pragma unroll
        for (int r = 0; r < 4; ++r) {            // D[row = kq + 4 r][col = i] = dW[unit kq + 4 r][input i]
            G[MT_W2 + (kq + 4 * r) * 16 + i] = dw2[r];
            if (kq + 4 * r < 11) G[MT_W3 + (kq + 4 * r) * 16 + i] = dw3[r];
        }
        if (kq == 0) {
            G[MT_W1 + 2 * i] = gw10; G[MT_W1 + 2 * i + 1] = gw11;
            G[MT_B1 + i] = gb1; G[MT_B2 + i] = gb2;
            if (i < 11) G[MT_B3 + i] = gb3;
        }
        __syncthreads();

        // ---- Adam (torch.optim.Adam: L2 folded into the gradient, lerp for the first moment, bias corrections by step count)
        {
            const double step_size = lr / (1.0 - mt_powi(0.9, e + 1u));
            const double bc2_sqrt = sqrt(1.0 - mt_powi(0.999, e + 1u));
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int p = lane + 64 * k;
                if (p < MT_PARAMS) {
                    const double w = P[p];
                    const double g = G[p] + mo.weight_decay * w;
                    am[k] = am[k] + (1.0 - 0.9) * (g - am[k]);
                    av[k] = av[k] * 0.999 + ((1.0 - 0.999) * g) * g;
                    const double denom = sqrt(av[k]) / bc2_sqrt + 1e-8;
                    P[p] = w + (-step_size * am[k]) / denom;
                }
            }
        }
        __syncthreads();
        mt_load_frags(P, f);

        // ---- validation with the updated weights
        loss = 0.0;
        for (uint32_t first = 0; first < mo.n_val; first += 64) {
            const MtRow row = mt_fetch_row(data, val_rows, first, mo.n_val, mo.target_mask);
            mt_forward(P, f, row, TA, TB, TC, XS);
            loss += mt_loss_row<false>(data, row, mo.huber_delta, 0.0, TC);
            __syncthreads();
        }
        val_loss = mt_wave_sum(loss) / mo.n_valid_val;
        if (history && lane == 0) {
            double* const h = history + ((size_t)blockIdx.x * history_epochs + e) * 3;
            h[0] = train_loss; h[1] = val_loss; h[2] = lr;
        }

        // ---- ReduceLROnPlateau (mode min, relative threshold 1e-4, cooldown 0, eps 1e-8)
        if (val_loss < sched_best * (1.0 - 1e-4)) { sched_best = val_loss; bad = 0; }
        else ++bad;
        if (bad > mo.sched_patience) {
            const double cut = lr * mo.sched_factor;
            const double next = cut > mo.min_lr ? cut : mo.min_lr;
            if (lr - next > 1e-8) { lr = next; ++reductions; }
            bad = 0;
        }
        // ---- early stopping on the validation loss; the best state is the output
        if (val_loss < best_val) {
            best_val = val_loss; best_epoch = e; stale = 0;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int p = lane + 64 * k;
                if (p < MT_PARAMS) best[p] = P[p];
            }
        } else ++stale;
        ++e;                                     // epochs run so far
        if (stale >= mo.patience || e == mo.epochs) break;       // wave-uniform: one wavefront, one model, every lane holds the same loss bits
    }
    if (lane == 0) {
        MlpTrainResultDev r;
        r.best_val_loss = best_val; r.last_train_loss = train_loss; r.last_val_loss = val_loss; r.last_lr = lr;
        r.best_epoch = best_epoch; r.epochs_run = e; r.lr_reductions = reductions; r.status = best_val < __builtin_inf() ? 0u : 1u;
        results[blockIdx.x] = r;
    }
}

}  // namespace owdev
