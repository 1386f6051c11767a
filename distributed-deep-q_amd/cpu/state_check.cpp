// The CPU twin's ddq_state_* (include/ddq_hip.h) under the sanitizers: the
// section walk, the range checks and the digest over odd sizes and offsets, and
// a write / commit round trip.  A program of its own, linked with cpu/twin.cpp:
//   make state_check
// (g++ -fopenmp -ffp-contract=off -fsanitize=address,undefined over both files).
// No GPU, nothing loaded into an interpreter.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/ddq_hip.h"

static int g_fail = 0;
#define CHECK(x)                                                     \
  do {                                                               \
    if (!(x)) {                                                      \
      printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #x);            \
      ++g_fail;                                                      \
    }                                                                \
  } while (0)

static uint64_t mix(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// the definition, word by word, on a copy padded with zeros
static uint64_t digest(const std::vector<uint8_t>& b) {
  const uint64_t n = b.size(), K = (n + 7) / 8;
  std::vector<uint8_t> p(K * 8, 0);
  if (n) memcpy(p.data(), b.data(), n);
  uint64_t d = mix(n);
  for (uint64_t k = 0; k < K; ++k) {
    uint64_t w;
    memcpy(&w, p.data() + 8 * k, 8);   // little-endian host
    d += mix(w ^ ((k + 1) * 0x9E3779B97F4A7C15ull));
  }
  return d;
}

static ddq_ctx* make(int64_t cap, bool adam, bool prio, int S = 16, int B = 4) {
  ddq_net_desc d{B, S, 4, 4, 0.85f};
  ddq_ctx* c = nullptr;
  CHECK(ddq_create(&c, 0, &d) == DDQ_OK);
  if (adam) {
    ddq_adam_cfg a{0.9f, 0.999f, 1e-8f, 1.0f};
    CHECK(ddq_set_adam(c, &a) == DDQ_OK);
  }
  CHECK(ddq_replay_create(c, cap) == DDQ_OK);
  std::vector<uint8_t> st((size_t)cap * 4 * S * S), ac(cap), nt(cap);
  std::vector<int16_t> rw(cap);
  uint64_t r = (uint64_t)cap;
  for (auto& v : st) v = (uint8_t)(r = mix(r));
  for (int64_t i = 0; i < cap; ++i) {
    ac[i] = (uint8_t)(mix(r + i) & 3);
    rw[i] = (int16_t)((int)(mix(r ^ i) % 3) - 1);
    nt[i] = (uint8_t)(mix(r * 3 + i) % 10 != 0);
  }
  CHECK(ddq_replay_import(c, st.data(), ac.data(), rw.data(), nt.data(), cap, cap / 2, cap) == DDQ_OK);
  if (prio) {
    ddq_priority_cfg p{1, 0.6f, 0.4f, 0.01f};
    CHECK(ddq_replay_set_priority(c, &p) == DDQ_OK);
  }
  return c;
}

static std::vector<ddq_state_section> sections(ddq_ctx* c) {
  int32_t n = 0;
  CHECK(ddq_state_sections(c, nullptr, 0, &n) == DDQ_OK);
  std::vector<ddq_state_section> s((size_t)n);
  CHECK(ddq_state_sections(c, s.data(), n - 1, &n) == DDQ_EINVAL);   // cap too small
  CHECK(ddq_state_sections(c, s.data(), n, &n) == DDQ_OK);
  return s;
}

static void walk(int64_t cap) {
  ddq_ctx* c = make(cap, true, cap >= 9);
  const auto secs = sections(c);
  CHECK(secs.size() == (cap >= 9 ? 11u : 10u));
  CHECK(!strcmp(secs[0].name, "config") && secs[0].bytes == 64);
  for (const auto& s : secs) {
    // exactly-sized heap buffers: a byte too many read or written is the sanitizer's
    std::vector<uint8_t> whole((size_t)s.bytes);
    CHECK(ddq_state_read(c, s.name, 0, whole.data(), s.bytes) == DDQ_OK);
    CHECK(digest(whole) == s.digest);
    uint64_t d = 0;
    CHECK(ddq_state_digest(c, s.name, &d) == DDQ_OK && d == s.digest);
    // odd ranges
    const int64_t offs[] = {0, 1, 7, s.bytes / 2, s.bytes - 1};
    const int64_t lens[] = {1, 3, 8, 17, s.bytes};
    for (int64_t o : offs)
      for (int64_t l : lens) {
        if (o < 0 || o >= s.bytes) continue;
        std::vector<uint8_t> part((size_t)l);
        const int rc = ddq_state_read(c, s.name, o, part.data(), l);
        if (o + l <= s.bytes) {
          CHECK(rc == DDQ_OK && !memcmp(part.data(), whole.data() + o, (size_t)l));
        } else {
          CHECK(rc == DDQ_EINVAL);
        }
      }
    uint8_t one = 0;
    CHECK(ddq_state_read(c, s.name, s.bytes, &one, 1) == DDQ_EINVAL);
    CHECK(ddq_state_read(c, s.name, -1, &one, 1) == DDQ_EINVAL);
    CHECK(ddq_state_read(c, s.name, 0, &one, 0) == DDQ_EINVAL);
    CHECK(ddq_state_read(c, s.name, 0, &one, s.bytes + 1) == DDQ_EINVAL);
    CHECK(ddq_state_write(c, s.name, 1, whole.data(), s.bytes) == DDQ_EINVAL);
    CHECK(ddq_state_write(c, s.name, 0, whole.data(), s.bytes + 1) == DDQ_EINVAL);
  }
  uint8_t one = 0;
  CHECK(ddq_state_read(c, "nonsense", 0, &one, 1) == DDQ_EINVAL);
  CHECK(ddq_state_read(c, nullptr, 0, &one, 1) == DDQ_EINVAL);
  CHECK(ddq_state_commit(c) == DDQ_OK);   // nothing written: a no-op
  ddq_destroy(c);
}

// every section of `from` into `to` in odd-sized pieces, then the digests agree
static void round_trip(int64_t cap) {
  ddq_ctx* from = make(cap, true, cap >= 9);
  ddq_ctx* to = make(cap, true, cap >= 9);
  // make `from` differ: another head and parameters
  std::vector<float> th((size_t)ddq_num_params(from));
  for (size_t i = 0; i < th.size(); ++i) th[i] = (float)((int)(mix(i) % 2001) - 1000) * 1e-3f;
  CHECK(ddq_set_params(from, 0, th.data(), (int64_t)th.size(), 0) == DDQ_OK);
  const auto secs = sections(from);
  for (const auto& s : secs) {
    std::vector<uint8_t> whole((size_t)s.bytes);
    CHECK(ddq_state_read(from, s.name, 0, whole.data(), s.bytes) == DDQ_OK);
    if (!strcmp(s.name, "config")) {
      CHECK(ddq_state_write(to, s.name, 0, whole.data(), s.bytes) == DDQ_OK);
      CHECK(ddq_state_write(to, s.name, 0, whole.data(), s.bytes - 1) == DDQ_EINVAL);
      continue;
    }
    for (int64_t o = 0; o < s.bytes;) {
      const int64_t l = std::min<int64_t>(s.bytes - o, 1 + (int64_t)(mix((uint64_t)o) % 4099));
      std::vector<uint8_t> piece(whole.begin() + o, whole.begin() + o + l);
      CHECK(ddq_state_write(to, s.name, o, piece.data(), l) == DDQ_OK);
      o += l;
    }
  }
  float loss = 0.f;
  CHECK(ddq_forward_backward(to, &loss) == DDQ_ESTATE);   // restoring
  CHECK(ddq_state_commit(to) == DDQ_OK);
  const auto got = sections(to);
  CHECK(got.size() == secs.size());
  for (size_t i = 0; i < secs.size() && i < got.size(); ++i)
    CHECK(got[i].bytes == secs[i].bytes && got[i].digest == secs[i].digest);
  // a config that differs: another n-step length
  if (cap >= 9) {
    CHECK(ddq_replay_set_nstep(to, 2) == DDQ_OK);
    ddq_state_config k;
    CHECK(ddq_state_read(from, "config", 0, &k, sizeof(k)) == DDQ_OK);
    CHECK(ddq_state_write(to, "config", 0, &k, sizeof(k)) == DDQ_EINVAL);
    CHECK(strstr(ddq_last_error(to), "nstep") != nullptr);
  }
  ddq_destroy(from);
  ddq_destroy(to);
}

int main() {
  CHECK(sizeof(ddq_state_section) == 32 && sizeof(ddq_state_config) == 64 &&
        sizeof(ddq_state_counters) == 96);
  for (int64_t cap : {2, 3, 9, 257, 4099}) walk(cap);
  for (int64_t cap : {3, 257}) round_trip(cap);
  if (g_fail) {
    printf("state check: %d failures\n", g_fail);
    return 1;
  }
  printf("state check ok\n");
  return 0;
}
