// wave_probe_mix.hip — wave_probe.hip's second translation unit: kernels.h WITHOUT GROOVE_WELSH_CLASS_TU, as groove_hip.hip sees it,
// for the one probed routine that lives in that part (wave_sum, the mix bus).  Linked into libwave_probe.so beside wave_probe.hip.
#define WAVE_PROBE_MIX_TU 1
#include "wave_probe.hip"
