// The device model of the synaptic accumulator as the host hands it to the kernels, and the caller's parameter planes as the
// host checks them: what accum_kernels.hip, accum_trials.hip (float32, event-driven) and accum_frames.hip (float64,
// frame-driven) share.  Everything sits in an unnamed namespace: each of
// the translation units has its own copy, and DevF / DevD stay local to the unit whose kernel signatures name them.
#pragma once

#include <algorithm>
#include <cmath>

#include "nsof_internal.h"

namespace {

// The device model (PARAMS, DT of event_mem_sim.py:20-30) as the float32 kernels take it: every field of nsof_accum_params
// rounded to float32 ONCE on the host -- NumPy does the same to the Python scalars of PARAMS next to a float32 array -- and
// neg_lam = (float)(-ln(Roff / Ron)), the logarithm taken in double as np.log takes it.  Passed BY VALUE in the kernel
// arguments: uniform, so the fields sit in SGPRs; no __constant__ symbol is written per call and no pixel loads anything
// for them, and two accumulators with different devices run back to back on one context.
struct DevF {
    float voff, von, koff, kon, son, soff, bon, boff, alphaoff, alphaon, dt, ron, neg_lam;
};
// The same model for the float64 frame-driven path, with the two values that path forms on the host with the library's
// log / exp (std::log is no constant expression): lambda = ln(Roff / Ron) and r0 = ron / exp(-lambda * (1 - wini)), the
// resistance of the array before the first frame pair.
struct DevD {
    double voff, von, koff, kon, son, soff, bon, boff, alphaoff, alphaon, ron, lambda, wini, r0;
};
// The fitted device of the paper (event_mem_sim.py:20-34) as compile-time constants.  The hot kernels -- the fused updates,
// the tile walk, the float64 frame loop -- are instantiated per model kind: the fitted one takes an (almost) empty argument
// and folds these constants, so the default path runs the code it ran before the parameters became arguments (same bits,
// same time: measured, a run-time model cost the launch-bound scheme-2 groups 1.5-2.5 %); the other instantiation reads the
// argument.  NULL or default parameters are routed to the fitted instantiation (Model::fitted); per-pixel planes are the
// third kind (MapF below, FrameMaps in accum_frames.hip).
__host__ __device__ constexpr DevF fitted_f()
{
    return DevF{(float)-0.2, (float)0.1, (float)51.03, (float)-2.91, (float)0.2, (float)0.8, (float)-5.12, (float)3.10,
                1.f, 1.f, (float)5e-4, 163305.f, -0x1.473018p+1f /* (float)-ln(2104377 / 163305) */};
}
__host__ __device__ constexpr DevD fitted_d()
{
    return DevD{-0.2, 0.1, 51.03, -2.91, 0.2, 0.8, -5.12, 3.10, 1.0, 1.0, 163305.0, 0.0 /* lambda, r0: see FittedD */, 0.5, 0.0};
}
// Per-pixel parameter maps (nsof_accum_set_param_maps): the third kind of model.  The voltages are fixed per accumulator, so
// everything a pixel's update needs is formed ONCE by k_setup_maps -- the active and the silent Drive (ka, s, b: 12 bytes
// each, dt stays a scalar) and the pair (ron, neg_lam) of its resistance -- and the hot kernels load a pixel's drive where
// they formed one from SGPRs: 12 bytes per driven pixel, nothing for an idle one.
struct MapF {
    const float* act;    // [npx][3]: drive_of(active voltage, the pixel's DevF)
    const float* sil;    // [npx][3]: drive_of(silent_v, the pixel's DevF)
    const float2* res;   // [npx]: (ron, neg_lam)
    float dt;
};

// event_mem_sim.py:20-34
inline nsof_accum_params default_params()
{
    nsof_accum_params p;
    p.alphaoff = 1; p.alphaon = 1; p.voff = -0.2; p.von = 0.1; p.koff = 51.03; p.kon = -2.91; p.son = 0.2; p.soff = 0.8;
    p.bon = -5.12; p.boff = 3.10; p.Ron = 163305.0; p.Roff = 2104377.0; p.wini = 0.5;
    p.dt = 5e-4;
    p.refractory_us = 800;
    return p;
}

// The double fields of nsof_accum_params by NSOF_ACCUM_KEY_*.
const char* const kKeyNames[NSOF_ACCUM_KEY_COUNT] = {"alphaoff", "alphaon", "voff", "von", "koff", "kon", "son", "soff", "bon",
                                                     "boff", "Ron", "Roff", "wini"};

// The domain of one parameter value: why `v` cannot be the value of `key` (the tail of a message), or nullptr where it can.
// A double (a scalar of nsof_accum_params, a float64 plane) is tested as the double AND as the float32 it rounds to where
// the float32 kernels divide by it or compare with it (voff, von, Ron); a float plane is its own float32.
template <class T>
const char* key_value_refused(int key, T v)
{
    const float vf = (float)v;
    if (!std::isfinite(v) || !std::isfinite(vf)) return "is not a finite float32";
    switch (key) {
    case NSOF_ACCUM_KEY_VOFF: return v < 0 && vf < 0.f ? nullptr : "must be negative (voff < 0 < von)";
    case NSOF_ACCUM_KEY_VON: return v > 0 && vf > 0.f ? nullptr : "must be positive (voff < 0 < von)";
    case NSOF_ACCUM_KEY_SON:
    case NSOF_ACCUM_KEY_SOFF:
    case NSOF_ACCUM_KEY_WINI: return v >= 0 && v <= 1 ? nullptr : "lies outside [0, 1]";
    case NSOF_ACCUM_KEY_RON: return v > 0 && vf > 0.f ? nullptr : "must be positive";
    case NSOF_ACCUM_KEY_ROFF: return v > 0 ? nullptr : "must be positive";
    default: return nullptr;
    }
}

// A parameter set the kernels can run (NULL: the defaults), with its float32 and float64 device forms; everything else is
// refused before anything is launched.
struct Model {
    nsof_accum_params prm;
    DevF f;
    DevD d;
    float wini_f;
    bool fitted;   // every field equals the fitted device's: the fitted kernel instantiations apply
    // per-pixel parameter maps (nsof_accum_set_param_maps; the planes belong to the accumulator's ParamMaps)
    bool mapped = false;
    MapF map{nullptr, nullptr, nullptr, 0.f};
};
inline int model_of(nsof_ctx* ctx, const nsof_accum_params* in, Model* m)
{
    const nsof_accum_params p = in ? *in : default_params();
    const double fields[NSOF_ACCUM_KEY_COUNT] = {p.alphaoff, p.alphaon, p.voff, p.von, p.koff, p.kon, p.son, p.soff, p.bon, p.boff,
                                                 p.Ron, p.Roff, p.wini};
    // every field finite first, then the domains: with several bad fields the first non-finite one is named
    for (int k = 0; k < NSOF_ACCUM_KEY_COUNT; k++)
        if (!std::isfinite(fields[k]) || !std::isfinite((float)fields[k]))
            return nsof_set_error(ctx, NSOF_EINVAL, "accumulator parameter %s = %g is not a finite float32", kKeyNames[k], fields[k]);
    if (!std::isfinite(p.dt) || !std::isfinite((float)p.dt))
        return nsof_set_error(ctx, NSOF_EINVAL, "accumulator parameter dt = %g is not a finite float32", p.dt);
    for (int k = 0; k < NSOF_ACCUM_KEY_COUNT; k++)
        if (const char* why = key_value_refused(k, fields[k]))
            return nsof_set_error(ctx, NSOF_EINVAL, "accumulator parameter %s = %g %s", kKeyNames[k], fields[k], why);
    if (!(p.dt > 0) || !((float)p.dt > 0.f)) return nsof_set_error(ctx, NSOF_EINVAL, "accumulator parameters: dt %g must be positive", p.dt);
    if (p.refractory_us < 0)
        return nsof_set_error(ctx, NSOF_EINVAL, "accumulator parameters: refractory_us %lld is negative", (long long)p.refractory_us);
    const double lambda = std::log(p.Roff / p.Ron);
    if (!std::isfinite(lambda)) return nsof_set_error(ctx, NSOF_EINVAL, "accumulator parameters: ln(Roff / Ron) is not finite");
    m->prm = p;
    m->f = DevF{(float)p.voff, (float)p.von, (float)p.koff, (float)p.kon, (float)p.son, (float)p.soff, (float)p.bon, (float)p.boff,
                (float)p.alphaoff, (float)p.alphaon, (float)p.dt, (float)p.Ron, (float)(-lambda)};
    m->d = DevD{p.voff, p.von, p.koff, p.kon, p.son, p.soff, p.bon, p.boff, p.alphaoff, p.alphaon, p.Ron, lambda, p.wini,
                p.Ron / std::exp(-lambda * (1 - p.wini))};
    m->wini_f = (float)p.wini;
    // The model's own fields decide (dt as the float32 the kernels multiply by; refractory_us never reaches a kernel).  The
    // constants of fitted_f / fitted_d, neg_lam's literal included, are pinned by the tests that hold the default path to the
    // correctly rounded reference bit for bit.
    const nsof_accum_params q = default_params();
    m->fitted = p.alphaoff == q.alphaoff && p.alphaon == q.alphaon && p.voff == q.voff && p.von == q.von && p.koff == q.koff &&
                p.kon == q.kon && p.son == q.son && p.soff == q.soff && p.bon == q.bon && p.boff == q.boff && p.Ron == q.Ron &&
                p.Roff == q.Roff && p.wini == q.wini && (float)p.dt == (float)q.dt;
    return NSOF_OK;
}

// The caller's planes by key: plane[k] (nullptr: the key keeps its scalar) holds trials[k] trials, 1 or the call's n_trials.
template <class T>
struct PlaneSet {
    const T* plane[NSOF_ACCUM_KEY_COUNT] = {};
    int trials[NSOF_ACCUM_KEY_COUNT] = {};
    bool any = false;
    // the value of key k at (trial t, pixel i): the plane's, or `scalar`
    template <class S>
    S at(int k, S scalar, size_t t, size_t i, size_t npx) const
    {
        return plane[k] ? (S)plane[k][(trials[k] == 1 ? 0 : t) * npx + i] : scalar;
    }
    double lambda_at(const nsof_accum_params& sp, size_t t, size_t i, size_t npx) const
    {
        return std::log(at(NSOF_ACCUM_KEY_ROFF, sp.Roff, t, i, npx) / at(NSOF_ACCUM_KEY_RON, sp.Ron, t, i, npx));
    }
    int lambda_trials() const   // 0: lambda is the scalar
    {
        return std::max(trials[NSOF_ACCUM_KEY_RON], trials[NSOF_ACCUM_KEY_ROFF]);
    }
};

// How an entry point's refusals begin: "<call>: ..." for the plane list, "<map> <key>: ..." for a value ("<map>s" for Ron / Roff).
struct PlaneLabels {
    const char *call, *map;
};

// Everything about a plane list that can refuse a call, on the host, before anything is uploaded or launched: the counts,
// every key / plane / trial count of the list, then every value of every plane, in the order given, against the domain the
// scalars have (key_value_refused) -- so a plane is refused exactly where model_of refuses that scalar -- then ln(Roff / Ron)
// per (trial, pixel) wherever either is a plane.  `mo` holds the scalars of the unmapped keys; the planes are [trials][H][W].
template <class T>
int plane_set_of(nsof_ctx* ctx, PlaneLabels lb, const Model& mo, int height, int width, int n_trials, int n_maps, const int* keys,
                 const T* const* planes, const int* plane_trials, PlaneSet<T>* ps)
{
    if (n_trials < 1) return nsof_set_error(ctx, NSOF_EINVAL, "%s: %d trials (at least 1)", lb.call, n_trials);
    if (n_maps < 0 || n_maps > NSOF_ACCUM_KEY_COUNT || (n_maps > 0 && (!keys || !planes || !plane_trials)))
        return nsof_set_error(ctx, NSOF_EINVAL, "%s: %d maps (0..%d, with their keys, planes and trial counts)", lb.call, n_maps,
                              NSOF_ACCUM_KEY_COUNT);
    for (int j = 0; j < n_maps; j++) {
        const int k = keys[j];
        if (k < 0 || k >= NSOF_ACCUM_KEY_COUNT)
            return nsof_set_error(ctx, NSOF_EINVAL, "%s: key %d is no parameter (0..%d)", lb.call, k, NSOF_ACCUM_KEY_COUNT - 1);
        if (!planes[j]) return nsof_set_error(ctx, NSOF_EINVAL, "%s: the plane of %s is NULL", lb.call, kKeyNames[k]);
        if (ps->plane[k]) return nsof_set_error(ctx, NSOF_EINVAL, "%s: %s given twice", lb.call, kKeyNames[k]);
        if (plane_trials[j] != 1 && plane_trials[j] != n_trials)
            return nsof_set_error(ctx, NSOF_EINVAL, "%s: the plane of %s holds %d trials (1 or %d)", lb.call, kKeyNames[k],
                                  plane_trials[j], n_trials);
        ps->plane[k] = planes[j];
        ps->trials[k] = plane_trials[j];
        ps->any = true;
    }
    const size_t npx = (size_t)height * width, W = (size_t)width;
    for (int j = 0; j < n_maps; j++)
        for (size_t e = 0; e < (size_t)plane_trials[j] * npx; e++)
            if (const char* why = key_value_refused(keys[j], planes[j][e]))
                return nsof_set_error(ctx, NSOF_EINVAL, "%s %s: trial %zu, row %zu, column %zu = %g %s", lb.map, kKeyNames[keys[j]],
                                      e / npx, e % npx / W, e % W, (double)planes[j][e], why);
    for (size_t t = 0; t < (size_t)ps->lambda_trials(); t++) {
        const T* const pon = ps->plane[NSOF_ACCUM_KEY_RON] ? ps->plane[NSOF_ACCUM_KEY_RON] + (ps->trials[NSOF_ACCUM_KEY_RON] == 1 ? 0 : t) * npx : nullptr;
        const T* const poff = ps->plane[NSOF_ACCUM_KEY_ROFF] ? ps->plane[NSOF_ACCUM_KEY_ROFF] + (ps->trials[NSOF_ACCUM_KEY_ROFF] == 1 ? 0 : t) * npx : nullptr;
        for (size_t i = 0; i < npx; i++) {
            // (ln q is finite exactly for a finite q > 0 -- subnormal q included: decided without T * H * W logarithms)
            const double q = (poff ? (double)poff[i] : mo.prm.Roff) / (pon ? (double)pon[i] : mo.prm.Ron);
            if (!(q > 0 && std::isfinite(q)))
                return nsof_set_error(ctx, NSOF_EINVAL, "%ss Ron / Roff: ln(Roff / Ron) is not finite at trial %zu, row %zu, column %zu",
                                      lb.map, t, i / W, i % W);
        }
    }
    return NSOF_OK;
}

// silent_v inside the dead zone [voff, von] of EVERY pixel of EVERY trial (the float32 comparisons update_one makes): an idle
// pixel is then a bit-exact no-op.  The two thresholds are tested independently, so each plane is one flat pass.
inline bool silent_in_every_dead_zone(const PlaneSet<float>& ps, const DevF& f, float silent_v, size_t npx)
{
    auto every_value = [&](int k, float scalar, auto&& ok) {
        if (!ps.plane[k]) return ok(scalar);
        for (size_t e = 0; e < (size_t)ps.trials[k] * npx; e++)
            if (!ok(ps.plane[k][e])) return false;
        return true;
    };
    return every_value(NSOF_ACCUM_KEY_VOFF, f.voff, [&](float v) { return !(silent_v < v); }) &&
           every_value(NSOF_ACCUM_KEY_VON, f.von, [&](float v) { return !(silent_v > v); });
}
// The same rule with a silent voltage per trial: silent_v[t] inside the dead zone of every pixel of trial t, for EVERY t (a
// plane shared by the trials is trial t's).
inline bool silent_in_every_dead_zone(const PlaneSet<float>& ps, const DevF& f, const float* silent_v, int n_trials, size_t npx)
{
    for (size_t t = 0; t < (size_t)n_trials; t++) {
        const float sv = silent_v[t];
        auto every_value = [&](int k, float scalar, auto&& ok) {
            if (!ps.plane[k]) return ok(scalar);
            const float* q = ps.plane[k] + (ps.trials[k] == 1 ? 0 : t) * npx;
            for (size_t i = 0; i < npx; i++)
                if (!ok(q[i])) return false;
            return true;
        };
        if (!every_value(NSOF_ACCUM_KEY_VOFF, f.voff, [&](float v) { return !(sv < v); }) ||
            !every_value(NSOF_ACCUM_KEY_VON, f.von, [&](float v) { return !(sv > v); }))
            return false;
    }
    return true;
}

}  // namespace
