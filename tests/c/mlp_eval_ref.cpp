// Test-side CPU restatement of a render whose note-on MLP corrections are given at run time, over the oracle's headers, which it includes
// unchanged.  Three pieces, each in the reference's statement order:
//   1. MlpCorrections::infer (mlp_correction.rs:61-140) with the weights as arguments (the oracle's mlp_infer, ow_tables.hpp, reads the
//      baked constants);
//   2. Voice::note_on (voice.rs:28-142) taking a MlpCorrections (the oracle's takes a flag and infers itself, ow_voice.hpp);
//   3. the `preamp-bench render` job body (tools/preamp-bench/src/main.rs:371-549) around that voice, with the flags
//      owo_batch_render_job_ex takes.
// tests/mlp_eval_ref.py builds it with the oracle Makefile's flags and loads it with ctypes; it is the checker of ow_mlp_infer,
// ow_batch_render_corrected and ow_batch_render_mlp.
#include "ow_engine.hpp"

#include <cmath>
#include <cstdint>
#include <vector>

using namespace owo;

namespace {

struct Weights {       // mlp_weights.rs, same shapes and order (= ow_mlp_weights of include/openwurli_hip.h)
    double w1[16][2], b1[16], w2[16][16], b2[16], w3[11][16], b3[11], target_means[11], target_stds[11];
};

// mlp_correction.rs:61-140; raw (NULL or 11): the denormalised outputs before fade and clamps (written even where the fade is zero)
MlpCorrections infer(const Weights& w, int midi_note, double velocity, double* raw_out) {
    const double MIDI_MIN = 21.0, MIDI_MAX = 108.0;
    const double TRAIN_LO = 65.0, TRAIN_HI = 97.0, FADE = 12.0;
    const double midi = (double)midi_note;
    double fade;
    if (midi < TRAIN_LO) fade = rclamp((midi - (TRAIN_LO - FADE)) / FADE, 0.0, 1.0);
    else if (midi > TRAIN_HI) fade = rclamp(((TRAIN_HI + FADE) - midi) / FADE, 0.0, 1.0);
    else fade = 1.0;
    if (fade <= 0.0 && !raw_out) return mlp_identity();

    const double in0 = rclamp((midi - MIDI_MIN) / (MIDI_MAX - MIDI_MIN), 0.0, 1.0);
    const double in1 = rclamp(velocity, 0.0, 1.0);
    const double input[2] = {in0, in1};
    double h1[16], h2[16], raw[11];
    for (int i = 0; i < 16; ++i) {
        double sum = w.b1[i];
        for (int j = 0; j < 2; ++j) sum += w.w1[i][j] * input[j];
        h1[i] = sum > 0.0 ? sum : 0.0;
    }
    for (int i = 0; i < 16; ++i) {
        double sum = w.b2[i];
        for (int j = 0; j < 16; ++j) sum += w.w2[i][j] * h1[j];
        h2[i] = sum > 0.0 ? sum : 0.0;
    }
    for (int i = 0; i < 11; ++i) {
        double sum = w.b3[i];
        for (int j = 0; j < 16; ++j) sum += w.w3[i][j] * h2[j];
        raw[i] = sum * w.target_stds[i] + w.target_means[i];
    }
    if (raw_out) for (int i = 0; i < 11; ++i) raw_out[i] = raw[i];
    if (fade <= 0.0) return mlp_identity();
    MlpCorrections c;
    for (int h = 0; h < 5; ++h) c.freq_offsets_cents[h] = rclamp(raw[h] * fade, -100.0, 100.0);
    for (int h = 0; h < 5; ++h) {
        const double rd = rclamp(raw[5 + h], 0.3, 3.0);
        c.decay_offsets[h] = 1.0 + (rd - 1.0) * fade;
    }
    const double raw_ds = rclamp(raw[10], 0.7, 1.2);
    c.ds_correction = 1.0 + (raw_ds - 1.0) * fade;
    return c;
}

// voice.rs:28-142 with `corr` in place of the MlpCorrections the reference infers there
void note_on(Voice& v, int midi, double velocity, double sr, uint32_t seed, const MlpCorrections& corr) {
    const NoteParams params = note_params(midi);
    const double f0d = params.fundamental_hz * freq_detune((uint8_t)midi);
    double dwell[NUM_MODES], offs[NUM_MODES], amps[NUM_MODES];
    dwell_attenuation(velocity, f0d, params.mode_ratios, dwell);
    const double onset_time = onset_ramp_time(velocity, f0d);
    mode_amplitude_offsets((uint8_t)midi, offs);
    for (int i = 0; i < NUM_MODES; ++i) amps[i] = params.mode_amplitudes[i] * dwell[i] * offs[i];
    const double vel_exp = velocity_exponent(midi);
    const double vel_scale = std::pow(velocity_scurve(velocity), vel_exp);
    for (int i = 0; i < NUM_MODES; ++i) amps[i] *= vel_scale;

    double ratios[NUM_MODES], decay[NUM_MODES];
    for (int i = 0; i < NUM_MODES; ++i) { ratios[i] = params.mode_ratios[i]; decay[i] = params.mode_decay_rates[i]; }
    for (int h = 0; h < 5; ++h) ratios[1 + h] *= std::pow(2.0, corr.freq_offsets_cents[h] / 1200.0);
    for (int h = 0; h < 5; ++h) decay[1 + h] /= corr.decay_offsets[h];
    const double corrected_ds = pickup_displacement_scale(midi) * corr.ds_correction;

    v.reed.init(f0d, ratios, amps, decay, onset_time, velocity, sr, seed);
    v.pickup.init(sr);
    v.pickup.displacement_scale = corrected_ds;
    v.noise.init(velocity, f0d, sr, seed);

    const double base_output_scale = output_scale(midi, velocity);
    const double base_ds = pickup_displacement_scale(midi);
    double comp = 1.0;
    if (std::fabs(corr.ds_correction - 1.0) > 1e-6) {
        const double f0 = midi_to_freq(midi);
        const double HPF_FC = 2312.0;
        const double pb = pickup_rms_proxy(base_ds, f0, HPF_FC);
        const double pc = pickup_rms_proxy(corrected_ds, f0, HPF_FC);
        comp = (pc > 1e-10) ? std::sqrt(pb / pc) : 1.0;
    }
    v.post_pickup_gain = base_output_scale * comp;
    v.sample_rate = sr;
    v.midi_note = midi;
}

// main.rs:371-549 around that voice
std::vector<double> render_job(int note, int velocity_u8, double duration, double sr, const BatchJobOpts& o, const MlpCorrections& corr) {
    const bool do_os = sr < 88200.0;
    const double preamp_sr = do_os ? sr * 2.0 : sr;
    const double vel_norm = (double)velocity_u8 / 127.0;
    const uint32_t seed = (uint32_t)note * 2654435761u;
    Voice voice;
    note_on(voice, note, vel_norm, sr, seed, corr);
    if (o.has_displacement_scale) voice.pickup.displacement_scale = o.displacement_scale;     // main.rs:406-408: after note_on
    if (o.no_attack_noise) voice.noise.remaining = 0;                                         // main.rs:409-411
    const size_t n = (size_t)as_u64(duration * sr);
    std::vector<double> reed(n, 0.0);
    for (size_t off = 0; off < n; off += 1024) voice.render(reed.data() + off, std::min((size_t)1024, n - off));

    std::vector<double> pre(n, 0.0);
    if (o.no_preamp) {                                                                        // main.rs:425-427
        pre = reed;
    } else {
        DkPreamp legacy;
        MelangePreamp mel;
        if (o.preamp_kind) mel.init(preamp_sr); else legacy.init(preamp_sr);
        Tremolo trem;
        const bool use_trem = o.tremolo_depth > 0.0;                                          // main.rs:430-441
        if (use_trem) trem.init(o.tremolo_depth, preamp_sr);
        else if (o.preamp_kind) { mel.reset(); mel.set_ldr_resistance(o.r_ldr); }
        else { legacy.reset(); legacy.set_ldr_resistance(o.r_ldr); }
        auto step = [&](double x) -> double {
            if (use_trem) { const double r = trem.process(); if (o.preamp_kind) mel.set_ldr_resistance(r); else legacy.set_ldr_resistance(r); }
            return o.preamp_kind ? mel.process_sample(x) : legacy.process_sample(x);
        };
        if (do_os) {
            Oversampler os;
            for (size_t i = 0; i < n; ++i) {
                double up[2], proc[2], down[1];
                os.upsample_2x(&reed[i], 1, up);
                proc[0] = step(up[0]);
                proc[1] = step(up[1]);
                os.downsample_2x(proc, down, 1);
                pre[i] = down[0];
            }
        } else {
            for (size_t i = 0; i < n; ++i) pre[i] = step(reed[i]);
        }
    }
    PowerAmp pa;
    MelangePowerAmp mpa;
    if (o.power_amp_kind) { mpa.init(44100.0); if (o.no_rail_sag) mpa.set_rail_sag(false); }  // main.rs:480-483
    Speaker spk;
    spk.init(sr);
    spk.set_character(o.speaker_char);
    std::vector<double> out(n, 0.0);
    for (size_t i = 0; i < n; ++i) {
        const double att = pre[i] * o.volume * o.volume;
        const double amp = o.poweramp ? (o.power_amp_kind ? mpa.process(att) : pa.process(att)) : att;
        out[i] = spk.process(amp) * POST_SPEAKER_GAIN;
    }
    return out;
}

MlpCorrections from11(const double* c) {
    MlpCorrections m;
    for (int i = 0; i < 5; ++i) { m.freq_offsets_cents[i] = c[i]; m.decay_offsets[i] = c[5 + i]; }
    m.ds_correction = c[10];
    return m;
}
}  // namespace

extern "C" {
// weights: 529 doubles laid out as ow_mlp_weights.  out11: 5 cents, 5 decay ratios, ds.  raw11: NULL or the denormalised outputs.
void omr_infer(const double* weights, int midi, double velocity, double* out11, double* raw11) {
    const MlpCorrections c = infer(*(const Weights*)weights, midi, velocity, raw11);
    for (int i = 0; i < 5; ++i) { out11[i] = c.freq_offsets_cents[i]; out11[5 + i] = c.decay_offsets[i]; }
    out11[10] = c.ds_correction;
}
size_t omr_weights_doubles(void) { return sizeof(Weights) / sizeof(double); }

// opts and flags as owo_batch_render_job_ex (oracle/ow_oracle_capi.cpp); bit 0 of flags (mlp) is not looked at: corr11 is what the
// note-on takes
size_t omr_render(int note, int vel_u8, double dur_s, double sr, const double* opts, unsigned flags, int preamp_kind, int power_amp_kind,
                  const double* corr11, double* out, size_t cap) {
    BatchJobOpts o;
    o.volume = opts[0]; o.speaker_char = opts[1]; o.r_ldr = opts[2]; o.tremolo_depth = opts[3];
    o.has_displacement_scale = opts[4] == opts[4]; o.displacement_scale = opts[4];
    o.mlp = false; o.poweramp = flags & 2u; o.no_preamp = flags & 4u; o.no_attack_noise = flags & 8u; o.no_rail_sag = flags & 16u;
    o.preamp_kind = preamp_kind; o.power_amp_kind = power_amp_kind;
    const std::vector<double> v = render_job(note, vel_u8, dur_s, sr, o, from11(corr11));
    const size_t n = std::min(cap, v.size());
    for (size_t i = 0; i < n; ++i) out[i] = v[i];
    return v.size();
}
}  // extern "C"
