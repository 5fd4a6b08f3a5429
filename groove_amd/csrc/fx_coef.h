// fx_coef.h — the f64 coefficient formulas of the IIR effect kinds and the parameter laws in front of them, ONE text for the
// host (derive.h's `_h` functions call these) and the device (ctl_link.h: a control link onto a filter's cutoff, q or
// passband-ripple derives the lane's coefficients where they live).  Identical to the oracle's math; the expressions and
// their order are what tests/test_fx_coef_cpu.py pins bit for bit against derive.h's entry points.  Contraction is off in every function
// that multiplies and adds (GROOVE_NO_CONTRACT): the device then rounds as the host does, and what is left between the two sides is the
// math libraries' last place.
//
// Parameters arrive as the floats groove_fx_params holds, widened to f64 by the caller.
#pragma once
#include "dsp_core.h"

namespace groove {

// groove_fx_set_param's laws for the parameters that become coefficients
GROOVE_HD double fx_percent_to_frequency(double p) { return 25.0 * pow(800.0, p); }
GROOVE_HD double fx_q_law(double v) { GROOVE_NO_CONTRACT return v * v * 10.0 + 0.707; } /* denormalize_q; passband-ripple takes the same law */

GROOVE_HD void fx_rbj_lowpass(double f0, double q, double fs, double* c5) {
  GROOVE_NO_CONTRACT
  const double w0 = 2.0 * 3.14159265358979323846 * f0 / fs, cw = cos(w0), sw = sin(w0);
  const double alpha = sw / (2.0 * q), a0 = 1.0 + alpha;
  c5[0] = (1.0 - cw) / 2.0 / a0; c5[1] = (1.0 - cw) / a0; c5[2] = (1.0 - cw) / 2.0 / a0;
  c5[3] = -2.0 * cw / a0; c5[4] = (1.0 - alpha) / a0;
}
GROOVE_HD void fx_rbj_highpass(double f0, double q, double fs, double* c5) {
  GROOVE_NO_CONTRACT
  const double w0 = 2.0 * 3.14159265358979323846 * f0 / fs, cw = cos(w0), sw = sin(w0);
  const double alpha = sw / (2.0 * q), a0 = 1.0 + alpha;
  c5[0] = (1.0 + cw) / 2.0 / a0; c5[1] = -(1.0 + cw) / a0; c5[2] = (1.0 + cw) / 2.0 / a0;
  c5[3] = -2.0 * cw / a0; c5[4] = (1.0 - alpha) / a0;
}
// The remaining cookbook modes (doc/Audio-EQ-Cookbook.txt:113-198); parameter conventions: DSP_SPEC §4.
GROOVE_HD double fx_bw_octaves(double f0, double bw_hz) {
  GROOVE_NO_CONTRACT
  const double lo = f0 - 0.5 * bw_hz, hi = f0 + 0.5 * bw_hz;
  if (!(lo > 0.0) || hi / lo > 256.0) return 8.0;
  return log2(hi / lo);
}
GROOVE_HD void fx_rbj_norm(double b0, double b1, double b2, double a0, double a1, double a2, double* c5) {
  c5[0] = b0 / a0; c5[1] = b1 / a0; c5[2] = b2 / a0; c5[3] = a1 / a0; c5[4] = a2 / a0;
}
// Is `kind` one of the eight BiQuad 12 dB modes / one of the nine IIR kinds?
GROOVE_HD bool fx_kind_is_biquad12(uint32_t kind) {
  switch (kind) {
    case GROOVE_FX_BIQUAD_LP12: case GROOVE_FX_BIQUAD_HP12: case GROOVE_FX_BIQUAD_BP12: case GROOVE_FX_BIQUAD_BS12:
    case GROOVE_FX_BIQUAD_AP12: case GROOVE_FX_BIQUAD_PEAK12: case GROOVE_FX_BIQUAD_LSHELF12: case GROOVE_FX_BIQUAD_HSHELF12: return true;
    default: return false;
  }
}
GROOVE_HD bool fx_kind_is_filter(uint32_t kind) { return kind == GROOVE_FX_BIQUAD_LP24 || fx_kind_is_biquad12(kind); }
// Coefficients of any BiQuad 12 dB effect kind; false when `kind` is not one.
GROOVE_HD bool fx_rbj_for_kind(uint32_t kind, double cutoff_hz, double q, double bandwidth_hz, double db_gain, double fs, double* c5) {
  GROOVE_NO_CONTRACT
  const double pi = 3.14159265358979323846;
  const double f0 = cutoff_hz, w0 = 2.0 * pi * f0 / fs, cw = cos(w0), sw = sin(w0);
  switch (kind) {
    case GROOVE_FX_BIQUAD_LP12: fx_rbj_lowpass(f0, q, fs, c5); return true;
    case GROOVE_FX_BIQUAD_HP12: fx_rbj_highpass(f0, q, fs, c5); return true;
    case GROOVE_FX_BIQUAD_BP12: {
      const double al = sw * sinh(log(2.0) / 2.0 * fx_bw_octaves(f0, bandwidth_hz) * w0 / sw);
      fx_rbj_norm(al, 0.0, -al, 1.0 + al, -2.0 * cw, 1.0 - al, c5); return true;
    }
    case GROOVE_FX_BIQUAD_BS12: {
      const double al = sw * sinh(log(2.0) / 2.0 * fx_bw_octaves(f0, bandwidth_hz) * w0 / sw);
      fx_rbj_norm(1.0, -2.0 * cw, 1.0, 1.0 + al, -2.0 * cw, 1.0 - al, c5); return true;
    }
    case GROOVE_FX_BIQUAD_AP12: {
      const double al = sw / (2.0 * q);
      fx_rbj_norm(1.0 - al, -2.0 * cw, 1.0 + al, 1.0 + al, -2.0 * cw, 1.0 - al, c5); return true;
    }
    case GROOVE_FX_BIQUAD_PEAK12: {
      const double A = pow(10.0, db_gain / 40.0), al = sw / (2.0 * 0.70710678118654752440);
      fx_rbj_norm(1.0 + al * A, -2.0 * cw, 1.0 - al * A, 1.0 + al / A, -2.0 * cw, 1.0 - al / A, c5); return true;
    }
    case GROOVE_FX_BIQUAD_LSHELF12: {
      const double A = pow(10.0, db_gain / 40.0), t = 2.0 * sqrt(A) * (sw / 2.0 * sqrt(2.0));
      fx_rbj_norm(A * ((A + 1) - (A - 1) * cw + t), 2 * A * ((A - 1) - (A + 1) * cw), A * ((A + 1) - (A - 1) * cw - t),
                  (A + 1) + (A - 1) * cw + t, -2 * ((A - 1) + (A + 1) * cw), (A + 1) + (A - 1) * cw - t, c5);
      return true;
    }
    case GROOVE_FX_BIQUAD_HSHELF12: {
      const double A = pow(10.0, db_gain / 40.0), t = 2.0 * sqrt(A) * (sw / 2.0 * sqrt(2.0));
      fx_rbj_norm(A * ((A + 1) + (A - 1) * cw + t), -2 * A * ((A - 1) + (A + 1) * cw), A * ((A + 1) + (A - 1) * cw - t),
                  (A + 1) - (A - 1) * cw + t, 2 * ((A - 1) - (A + 1) * cw), (A + 1) - (A - 1) * cw - t, c5);
      return true;
    }
    default: return false;
  }
}
// out6 = b0,a1,a2 (section 1), b0,a1,a2 (section 2); y = b0 x + 2 b0 x1 + b0 x2 + a1 y1 + a2 y2
GROOVE_HD void fx_lp24_coeffs(double fc, double ripple, double fs, double* out6) {
  GROOVE_NO_CONTRACT
  if (fc > 0.49 * fs) fc = 0.49 * fs;
  if (fc < 1.0) fc = 1.0;
  const double k = tan(3.14159265358979323846 * fc / fs);
  double sg = sinh(ripple), cg = cosh(ripple);
  cg *= cg;
  const double c0 = 1.0 / (cg - 0.85355339059327376220), c1 = k * c0 * sg * 1.84775906502257351226;
  const double c2 = 1.0 / (cg - 0.14644660940672623780), c3 = k * c2 * sg * 0.76536686473017954346;
  const double K = k * k;
  const double a0 = 1.0 / (c1 + K + c0), a3 = 1.0 / (c3 + K + c2);
  out6[0] = a0 * K; out6[1] = 2.0 * (c0 - K) * a0; out6[2] = (c1 - K - c0) * a0;
  out6[3] = a3 * K; out6[4] = 2.0 * (c2 - K) * a3; out6[5] = (c3 - K - c2) * a3;
}

} // namespace groove
