// welsh_plan_check — plans Welsh banks on the CPU (groove_amd/csrc/welsh_plan.h), checks every plan's invariants and prints one
// line per bank: its name, the SHA-256 of the plan's bytes and a few counts.  Built and run by tests/test_welsh_plan_cpu.py.
//
//   welsh_plan_check <sample rate> <bank> [<bank> ...]        bank = name:f|-:file[:file2]
//
// `file` holds groove_welsh_params records, one per voice, as the caller of groove_bank_create_welsh would pass them.  The records
// are derived (derive.h derive_welsh), flagged with WF_FILTER_F32 where welsh_filter_f32_ok says so (`f`; `-`: no flag, as under
// GROOVE_F32_FILTER=0), put in the order welsh_patch_major_order chooses and planned.  With `file2` (the same bank after a
// control change) its records are then planned in the order the first plan chose, and that second plan is the one checked,
// hashed and counted.  Exit status 1 and a line on stderr for a violated invariant.
//
// THE DIGEST is SHA-256 over, in this order, little-endian, without padding between the parts:
//   u32 n, u32 n_vwaves, u8 tp_pairs, u8 tp_full_coef,
//   perm (u32 each; nothing when empty), inv (likewise),
//   records (WelshParams, n of them), cold (f64, 4 n),
//   waves (WaveDesc, n_vwaves of them),
//   wgs_of_kind (u32, kWgKinds),
//   sorted.list (u32 each), sorted.cls, sorted.base, sorted.f32 (u8 each), striped.list, striped.cls, striped.base, striped.f32,
//   mix_off (u32, 3), mix_cnt (u32, 3).
#include "groove_amd/csrc/welsh_plan.h"
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>

using namespace groove;

// ------------------------------------------------------------------ SHA-256 (FIPS 180-4)
struct Sha256 {
  uint32_t h[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au, 0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
  unsigned char buf[64];
  uint64_t len = 0;
  static uint32_t rotr(uint32_t x, int k) { return (x >> k) | (x << (32 - k)); }
  void block(const unsigned char* p) {
    static const uint32_t K[64] = {
        0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u, 0xd807aa98u, 0x12835b01u, 0x243185beu,
        0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u, 0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau,
        0x5cb0a9dcu, 0x76f988dau, 0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u, 0x27b70a85u,
        0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u, 0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u,
        0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u, 0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu,
        0x682e6ff3u, 0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};
    uint32_t w[64];
    for (int i = 0; i < 16; ++i) w[i] = (uint32_t)p[4 * i] << 24 | (uint32_t)p[4 * i + 1] << 16 | (uint32_t)p[4 * i + 2] << 8 | (uint32_t)p[4 * i + 3];
    for (int i = 16; i < 64; ++i) {
      const uint32_t s0 = rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3), s1 = rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10);
      w[i] = w[i - 16] + s0 + w[i - 7] + s1;
    }
    uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
    for (int i = 0; i < 64; ++i) {
      const uint32_t t1 = hh + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g)) + K[i] + w[i];
      const uint32_t t2 = (rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
      hh = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
    }
    h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
  }
  void add(const void* data, size_t bytes) {
    const unsigned char* p = static_cast<const unsigned char*>(data);
    for (size_t i = 0; i < bytes; ++i) {
      buf[len++ % 64] = p[i];
      if (len % 64 == 0) block(buf);
    }
  }
  template <class T> void add_vec(const std::vector<T>& v) { if (!v.empty()) add(v.data(), v.size() * sizeof(T)); }
  std::string hex() {
    const uint64_t bits = len * 8;
    const unsigned char one = 0x80, zero = 0;
    add(&one, 1);
    while (len % 64 != 56) add(&zero, 1);
    unsigned char be[8];
    for (int i = 0; i < 8; ++i) be[i] = (unsigned char)(bits >> (56 - 8 * i));
    add(be, 8);
    char out[65];
    for (int i = 0; i < 8; ++i) std::snprintf(out + 8 * i, 9, "%08x", h[i]);
    return out;
  }
};

static std::string plan_digest(const WelshPlan& p) {
  Sha256 s;
  const uint32_t n = (uint32_t)p.records.size();
  const uint8_t pairs = p.tp_pairs, full = p.tp_full_coef;
  s.add(&n, 4); s.add(&p.n_vwaves, 4); s.add(&pairs, 1); s.add(&full, 1);
  s.add_vec(p.perm); s.add_vec(p.inv);
  s.add_vec(p.records); s.add_vec(p.cold);
  s.add_vec(p.waves);
  s.add(p.wgs_of_kind, sizeof(p.wgs_of_kind));
  for (const WgLists* l : {&p.sorted, &p.striped}) { s.add_vec(l->list); s.add_vec(l->cls); s.add_vec(l->base); s.add_vec(l->f32); }
  s.add(p.mix_off, sizeof(p.mix_off)); s.add(p.mix_cnt, sizeof(p.mix_cnt));
  return s.hex();
}

// ------------------------------------------------------------------ records in, derived and flagged
static std::vector<groove_welsh_params> read_records(const std::string& path) {
  std::FILE* f = std::fopen(path.c_str(), "rb");
  if (!f) { std::fprintf(stderr, "cannot open %s\n", path.c_str()); std::exit(2); }
  std::vector<groove_welsh_params> v;
  groove_welsh_params r;
  while (std::fread(&r, sizeof(r), 1, f) == 1) v.push_back(r);
  std::fclose(f);
  return v;
}
// (the measurement of welsh_filter_f32_ok is ~0.6 ms: once per distinct filter description, as the library keeps it per bank)
struct FilterKey {
  float c0, d1, c2, d3, hz, start, end, depth;
  uint32_t bits;
  bool operator<(const FilterKey& o) const { return std::memcmp(this, &o, sizeof(FilterKey)) < 0; }
};
static void derive(const std::vector<groove_welsh_params>& in, double sr, bool flag, std::map<FilterKey, bool>& memo, std::vector<WelshParams>& P,
                   std::vector<WelshCold>& C) {
  P.resize(in.size()); C.resize(in.size());
  for (size_t v = 0; v < in.size(); ++v) {
    P[v] = derive_welsh(in[v], sr, C[v]);
    if (!flag) continue;
    const WelshParams& o = P[v];
    FilterKey k{};
    k.c0 = o.fc.c0; k.d1 = o.fc.d1; k.c2 = o.fc.c2; k.d3 = o.fc.d3; k.hz = o.cutoff_hz; k.start = o.cutoff_start; k.end = o.cutoff_end;
    k.depth = (o.flags & WF_LFO_CUTOFF) ? o.lfo_depth : 0.0f; k.bits = o.flags & (WF_RETUNE_ENV | WF_LFO_CUTOFF | WF_LFO_RESO | WF_COEF_WIDE);
    auto it = memo.find(k);
    if (it == memo.end()) it = memo.emplace(k, welsh_filter_f32_ok(o, sr)).first;
    if (it->second) P[v].flags |= WF_FILTER_F32;
  }
}

// ------------------------------------------------------------------ the invariants
static const char* g_bank = "";
#define REQUIRE(cond, ...) do { if (!(cond)) { std::fprintf(stderr, "%s: violated: %s — ", g_bank, #cond); std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); std::exit(1); } } while (0)

static bool same(const WelshParams& a, const WelshParams& b) { return std::memcmp(&a, &b, sizeof(WelshParams)) == 0; }
static uint32_t sort_key_of(const WelshParams& p) { // (kind, fp32 flag) of the workgroup a wave of this patch belongs in
  const int base = welsh_base_kind(p);
  int cl, c1, c2;
  welsh_body_classes(p, base, cl, c1, c2);
  return ((uint32_t)wg_kind_of(base, cl, c1, c2) << 1) | ((p.flags & WF_FILTER_F32) ? 1u : 0u);
}
static void check_lists_sized(const WgLists& l, size_t entries) {
  REQUIRE(l.list.size() == entries && l.cls.size() == entries && l.base.size() == entries && l.f32.size() == entries, "%zu entries", entries);
}

static void check_plan(const WelshPlan& p, const std::vector<WelshParams>& ext, const std::vector<WelshCold>& cold_ext) {
  const uint32_t n = (uint32_t)ext.size();
  // the internal-order records and cold values equal the external ones through perm; inv is perm's inverse
  REQUIRE(p.perm.empty() || p.perm.size() == n, "perm %zu", p.perm.size());
  REQUIRE(p.inv.size() == p.perm.size(), "inv %zu", p.inv.size());
  REQUIRE(p.records.size() == n && p.cold.size() == (size_t)4 * n, "records %zu cold %zu", p.records.size(), p.cold.size());
  std::vector<uint8_t> seen(n, 0);
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t v = p.perm.empty() ? i : p.perm[i];
    REQUIRE(v < n && !seen[v], "perm[%u] = %u", i, v);
    seen[v] = 1;
    REQUIRE(p.perm.empty() || p.inv[v] == i, "inv[perm[%u]]", i);
    REQUIRE(same(p.records[i], ext[v]), "record of lane %u", i);
    const double want[4] = {cold_ext[v].tune1, cold_ext[v].tune2, cold_ext[v].fixed1, cold_ext[v].fixed2};
    for (int w = 0; w < 4; ++w) REQUIRE(std::memcmp(&p.cold[(size_t)w * n + i], &want[w], 8) == 0, "cold[%d][%u]", w, i);
  }
  // tp_pairs, tp_full_coef: as defined
  bool pairs = true, full = false;
  for (uint32_t i = 0; i + 1 < n; i += 2) pairs = pairs && same(p.records[i], p.records[i + 1]);
  for (uint32_t i = 0; i < n; ++i) full = full || (p.records[i].flags & WF_LFO_RESO);
  REQUIRE(p.tp_pairs == pairs && p.tp_full_coef == full, "pairs %d full %d", (int)pairs, (int)full);
  REQUIRE(p.n_vwaves == p.waves.size() && p.n_vwaves % kPlanWaves == 0, "n_vwaves %u", p.n_vwaves);
  const uint32_t wgs = p.n_vwaves / kPlanWaves;
  uint32_t sum = 0;
  for (uint32_t c : p.wgs_of_kind) sum += c;
  REQUIRE(sum == wgs, "wgs_of_kind sums to %u of %u", sum, wgs);
  const KindSlices ks = kind_slices(p.wgs_of_kind);
  check_lists_sized(p.sorted, wgs);
  check_lists_sized(p.striped, ks.n_spec);
  if (p.n_vwaves == 0) { // the per-lane kernel: no list, no section
    for (int s = 0; s < 3; ++s) REQUIRE(p.mix_off[s] == 0 && p.mix_cnt[s] == 0, "section %d", s);
    // ... taken only when the runs are short in this order
    REQUIRE(!runs_are_long(count_virtual_waves(p.records, n, [](uint32_t i) { return i; }), n), "per-lane with long runs");
    return;
  }
  // every voice lies in exactly one wave of non-zero count; a wave's voices have its record; no wave has more than 64 voices;
  // pad waves have count 0 and a valid vbase
  std::vector<uint8_t> covered(n, 0);
  for (const WaveDesc& w : p.waves) {
    REQUIRE(w.count <= 64 && w.vbase < n && (size_t)w.vbase + w.count <= n, "wave at %u count %u", w.vbase, w.count);
    for (uint32_t v = w.vbase; v < w.vbase + w.count; ++v) {
      REQUIRE(!covered[v], "voice %u in two waves", v);
      covered[v] = 1;
      REQUIRE(same(p.records[v], w.p), "voice %u differs from its wave", v);
    }
  }
  for (uint32_t v = 0; v < n; ++v) REQUIRE(covered[v], "voice %u in no wave", v);
  // the four waves of a workgroup have one kind and one fp32 flag (padding: a wave of the same patch kind)
  std::vector<uint32_t> key_of_wg(wgs);
  for (uint32_t g = 0; g < wgs; ++g) {
    key_of_wg[g] = sort_key_of(p.waves[(size_t)g * kPlanWaves].p);
    REQUIRE(p.waves[(size_t)g * kPlanWaves].count > 0, "workgroup %u starts with a pad wave", g);
    for (int k = 1; k < kPlanWaves; ++k) REQUIRE(sort_key_of(p.waves[(size_t)g * kPlanWaves + k].p) == key_of_wg[g], "workgroup %u wave %d", g, k);
  }
  // the sorted list: a permutation of 0 .. wgs - 1, non-decreasing in (kind, flag); cls / base / f32 are those of the workgroup named
  auto check_entry = [&](const WgLists& l, uint32_t i) {
    const uint32_t g = l.list[i];
    REQUIRE(g < wgs, "entry %u names workgroup %u", i, g);
    const uint32_t kind = key_of_wg[g] >> 1;
    REQUIRE(l.cls[i] == kind % kClassCombos && l.base[i] == kind / kClassCombos && l.f32[i] == (key_of_wg[g] & 1u), "entry %u", i);
  };
  std::vector<uint8_t> listed(wgs, 0);
  std::vector<uint32_t> count_of_kind(kWgKinds, 0);
  for (uint32_t i = 0; i < wgs; ++i) {
    check_entry(p.sorted, i);
    REQUIRE(!listed[p.sorted.list[i]], "workgroup %u listed twice", p.sorted.list[i]);
    listed[p.sorted.list[i]] = 1;
    REQUIRE(i == 0 || key_of_wg[p.sorted.list[i - 1]] <= key_of_wg[p.sorted.list[i]], "sorted list out of order at %u", i);
    count_of_kind[key_of_wg[p.sorted.list[i]] >> 1] += 1;
  }
  for (int k = 0; k < kWgKinds; ++k) REQUIRE(count_of_kind[k] == p.wgs_of_kind[k], "wgs_of_kind[%d]", k);
  // kind_slices: offsets and counts tile the list, base kind by base kind; n_spec is the first four kinds' total
  uint32_t at = 0;
  for (int b = 0; b < kBaseKinds; ++b) {
    REQUIRE(ks.offset[b] == at, "offset[%d]", b);
    for (uint32_t i = at; i < at + ks.count[b]; ++i) REQUIRE(p.sorted.base[i] == b, "entry %u not of base kind %d", i, b);
    at += ks.count[b];
  }
  REQUIRE(at == wgs && ks.n_spec == ks.count[0] + ks.count[1] + ks.count[2] + ks.count[3], "n_spec %u", ks.n_spec);
  // the three mix sections: slots s, s + 3, ... of the first n_spec entries of the sorted list, back to back in the striped lists
  at = 0;
  for (uint32_t s = 0; s < 3; ++s) {
    REQUIRE(p.mix_off[s] == at && p.mix_cnt[s] == (ks.n_spec + 2 - s) / 3, "section %u: off %u cnt %u", s, p.mix_off[s], p.mix_cnt[s]);
    for (uint32_t j = 0; j < p.mix_cnt[s]; ++j, ++at) {
      const uint32_t from = s + 3 * j;
      REQUIRE(p.striped.list[at] == p.sorted.list[from] && p.striped.cls[at] == p.sorted.cls[from] && p.striped.base[at] == p.sorted.base[from] &&
                  p.striped.f32[at] == p.sorted.f32[from], "section %u entry %u", s, j);
      check_entry(p.striped, at);
      REQUIRE(j == 0 || key_of_wg[p.striped.list[at - 1]] <= key_of_wg[p.striped.list[at]], "section %u out of order at %u", s, j);
    }
  }
  REQUIRE(at == ks.n_spec, "sections hold %u of %u", at, ks.n_spec);
}

static void print_bank(const char* name, const WelshPlan& p, bool order_kept) {
  const uint32_t n = (uint32_t)p.records.size();
  uint32_t pads = 0, flagged = 0, kinds = 0, odd_kinds = 0;
  for (const WaveDesc& w : p.waves) pads += w.count == 0;
  for (const WelshParams& r : p.records) flagged += (r.flags & WF_FILTER_F32) != 0;
  for (uint32_t c : p.wgs_of_kind) kinds += c != 0;
  { // kinds whose wave count is no multiple of four: those with padding
    for (uint32_t g = 0; g < p.n_vwaves / kPlanWaves; ++g) odd_kinds += p.waves[(size_t)g * kPlanWaves + kPlanWaves - 1].count == 0;
  }
  const KindSlices ks = kind_slices(p.wgs_of_kind);
  uint32_t f32_wgs = 0;
  for (uint8_t f : p.sorted.f32) f32_wgs += f;
  std::printf("%s %s n=%u regrouped=%d order_kept=%d waves=%u pads=%u padded_groups=%u wgs=%u n_spec=%u kinds=%u base=%u,%u,%u,%u,%u,%u mix=%u,%u,%u tp_pairs=%d tp_full_coef=%d "
              "flagged=%u f32_wgs=%u\n",
              name, plan_digest(p).c_str(), n, (int)!p.perm.empty(), (int)order_kept, p.n_vwaves - pads, pads, odd_kinds, p.n_vwaves / kPlanWaves, ks.n_spec, kinds,
              ks.count[0], ks.count[1], ks.count[2], ks.count[3], ks.count[4], ks.count[5], p.mix_cnt[0], p.mix_cnt[1], p.mix_cnt[2], (int)p.tp_pairs,
              (int)p.tp_full_coef, flagged, f32_wgs);
}

int main(int argc, char** argv) {
  if (argc < 3) { std::fprintf(stderr, "usage: %s <sample rate> name:f|-:file[:file2] ...\n", argv[0]); return 2; }
  const double sr = std::atof(argv[1]);
  { // FIPS 180-4's own example, so that a digest printed below is what any SHA-256 gives for those bytes
    Sha256 s;
    s.add("abc", 3);
    if (s.hex() != "ba7816bf8f01cfea414140de5dae2223b00361a396177a9cb410ff61f20015ad") { std::fprintf(stderr, "SHA-256 self-check failed\n"); return 3; }
  }
  for (int a = 2; a < argc; ++a) {
    std::vector<std::string> part;
    std::string spec = argv[a];
    for (size_t at = 0;;) {
      const size_t c = spec.find(':', at);
      part.push_back(spec.substr(at, c == std::string::npos ? c : c - at));
      if (c == std::string::npos) break;
      at = c + 1;
    }
    if (part.size() < 3 || part.size() > 4) { std::fprintf(stderr, "bad bank: %s\n", argv[a]); return 2; }
    g_bank = part[0].c_str();
    const bool flag = part[1] == "f";
    std::map<FilterKey, bool> memo;
    std::vector<WelshParams> P;
    std::vector<WelshCold> C;
    derive(read_records(part[2]), sr, flag, memo, P, C);
    WelshPlan plan = welsh_plan(P, C, welsh_patch_major_order(P));
    check_plan(plan, P, C);
    bool order_kept = false;
    if (part.size() == 4) { // the bank after a control change: the state stays where it is, so does the lane order
      const std::vector<uint32_t> perm = plan.perm;
      derive(read_records(part[3]), sr, flag, memo, P, C);
      REQUIRE(P.size() == plan.records.size(), "file2 holds %zu voices", P.size());
      plan = welsh_plan(P, C, perm);
      check_plan(plan, P, C);
      REQUIRE(plan.perm == perm, "the kept order changed");
      order_kept = true;
    }
    print_bank(g_bank, plan, order_kept);
  }
  return 0;
}
