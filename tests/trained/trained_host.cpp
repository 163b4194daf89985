// trained_host.cpp -- the CPU model of Trained_Compression's decoder: zip-ada_amd/csrc/zada_unlzma_logic.h compiled for the host with one "lane", a
// stream (5-byte header, no size field) decoded in one piece, or stopped at a symbol boundary and started again from the state it left, as the
// device does it (zada_unlzma.hip, k_unlzma_trained): the second half sees a fresh copy of the model, a fresh output buffer that holds the text so
// far, and only the input from the boundary on.  tests/_trained.py builds it into libtrained_host.so and calls it through ctypes; with
// -DTRAINED_MAIN it is a program of its own (built with -fsanitize=address,undefined) that checks one stream file at many boundaries.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../zip-ada_amd/csrc/zada_unlzma_logic.h"

namespace {
using namespace zada;

void leave(const UlzResult &R, uint64_t in_base, uint64_t *res8) {
  res8[0] = R.out_len; res8[1] = R.rc ? 0 : R.in_used + in_base; res8[2] = R.rule; res8[3] = R.in_pos + in_base; res8[4] = 0; res8[5] = R.out_pos; res8[6] = R.end; res8[7] = 0;
}

// The stream in exact-size heap copies (a sanitizer sees a byte too many).  in_limit / symbols: UlzStop; both ~0: one piece.
// fork3 = input bytes taken, bytes written at the boundary, 1 if the decoder stopped there.  An in_limit below ten -- the header and the range
// coder's five bytes reach beyond it -- is no fork at all, as zada_trained_open_decoder has it.
int decode(const uint8_t *in, uint64_t n_in, uint8_t *out, uint64_t cap, uint32_t eos, uint64_t in_limit, uint64_t symbols, uint64_t *res8, uint64_t *fork3) {
  const bool whole = (in_limit == ~0ull && symbols == ~0ull) || in_limit < 10;
  const uint64_t n1 = whole || in_limit > n_in ? n_in : in_limit;
  uint8_t *src = (uint8_t *)malloc(n1 ? n1 : 1);
  uint8_t *dst = (uint8_t *)malloc(cap ? cap : 1);
  uint16_t *probs = (uint16_t *)malloc(ULZ_NPROBS * 2);
  if (!src || !dst || !probs) { free(src); free(dst); free(probs); return -2; }
  if (n1) memcpy(src, in, n1);
  fork3[0] = fork3[1] = fork3[2] = 0;
  UlzResult R;
  UlzProps P{};
  const uint32_t rule = ulz_props5(src, n1, P);
  if (rule) { ulz_fail(R, rule, n1 < 5 ? n1 : 0, 0); leave(R, 0, res8); free(src); free(dst); free(probs); return R.rc; }
  const uint64_t nl = ulz_lit_elems(P);
  uint16_t *lit = (uint16_t *)malloc((size_t)nl * 2);
  if (!lit) { free(src); free(dst); free(probs); return -2; }
  for (uint32_t i = 0; i < ULZ_NPROBS; i++) probs[i] = ULZ_PROB_INIT;
  for (uint64_t i = 0; i < nl; i++) lit[i] = ULZ_PROB_INIT;
  UlzHostIO io{src, n1, 5, false, probs, lit, dst};
  UlzFork F{};
  const UlzStop stop{in_limit, symbols};
  if (whole) ulz_decode(io, P, cap, eos, R);
  else ulz_decode_f<true>(io, P, cap, eos, R, nullptr, &stop, &F);
  uint64_t in_base = 0;
  if (R.rc == 0 && R.end == ULZ_END_FORK) {
    // the second half: what the device hands to an entry's wave
    fork3[0] = F.in_pos; fork3[1] = F.out_pos; fork3[2] = 1;
    const uint64_t n2 = n_in - F.in_pos;
    uint8_t *src2 = (uint8_t *)malloc(n2 ? n2 : 1);
    uint8_t *dst2 = (uint8_t *)malloc(cap ? cap : 1);
    uint16_t *probs2 = (uint16_t *)malloc(ULZ_NPROBS * 2);
    uint16_t *lit2 = (uint16_t *)malloc((size_t)nl * 2);
    if (!src2 || !dst2 || !probs2 || !lit2) { free(src2); free(dst2); free(probs2); free(lit2); free(src); free(dst); free(probs); free(lit); return -2; }
    if (n2) memcpy(src2, in + F.in_pos, n2);
    if (F.out_pos) memcpy(dst2, dst, F.out_pos);
    memcpy(probs2, probs, ULZ_NPROBS * 2);
    memcpy(lit2, lit, (size_t)nl * 2);
    UlzHostIO io2{src2, n2, 0, false, probs2, lit2, dst2};
    const UlzFork start = F;
    ulz_decode_f<true>(io2, P, cap, eos, R, &start, nullptr, &F);
    in_base = start.in_pos;
    if (R.out_len) memcpy(out, dst2, R.out_len);
    free(src2); free(dst2); free(probs2); free(lit2);
  } else if (R.out_len) memcpy(out, dst, R.out_len);
  leave(R, in_base, res8);
  free(src); free(dst); free(probs); free(lit);
  return R.rc;
}
}  // namespace

extern "C" {

// returns 0 or -7 (ZADA_E_DATA); res8 = out_len, in_used, rule, input byte, 0, output position, how the stream ended (1: marker, 2: without), 0; out
// receives out_len bytes
int tm_decode(const uint8_t *in, uint64_t n_in, uint8_t *out, uint64_t cap, uint32_t eos, uint64_t *res8) {
  uint64_t f3[3];
  return decode(in, n_in, out, cap, eos, ~0ull, ~0ull, res8, f3);
}
int tm_decode_forked(const uint8_t *in, uint64_t n_in, uint8_t *out, uint64_t cap, uint32_t eos, uint64_t in_limit, uint64_t symbols, uint64_t *res8, uint64_t *fork3) {
  return decode(in, n_in, out, cap, eos, in_limit, symbols, res8, fork3);
}
const char *tm_rule_name(unsigned rule) { return zada::ulz_rule_name(rule); }
uint64_t tm_fork_margin() { return zada::ULZ_FORK_MARGIN; }

}

#ifdef TRAINED_MAIN
// trained_check FILE CAP [STEP]: the stream in FILE decoded in one piece and forked at every STEP-th input limit and at every STEP-th symbol
int main(int argc, char **argv) {
  if (argc < 3) { fprintf(stderr, "usage: %s stream cap [step]\n", argv[0]); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  std::vector<uint8_t> s;
  uint8_t buf[65536];
  for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) s.insert(s.end(), buf, buf + k);
  fclose(f);
  const uint64_t cap = strtoull(argv[2], nullptr, 10), step = argc > 3 ? strtoull(argv[3], nullptr, 10) : 1;
  std::vector<uint8_t> a(cap ? cap : 1), b(cap ? cap : 1);
  uint64_t ra[8], rb[8], f3[3], checked = 0, forked = 0;
  const int rca = tm_decode(s.data(), s.size(), a.data(), cap, 1, ra);
  for (int mode = 0; mode < 2; mode++) {
    const uint64_t top = mode == 0 ? s.size() + 2 * zada::ULZ_FORK_MARGIN : ra[5] + 2;      // (symbols <= bytes written + the marker)
    for (uint64_t v = 0; v <= top; v += step) {
      const int rcb = tm_decode_forked(s.data(), s.size(), b.data(), cap, 1, mode == 0 ? v : ~0ull, mode == 0 ? ~0ull : v, rb, f3);
      if (rca != rcb || memcmp(ra, rb, sizeof ra) || (ra[0] && memcmp(a.data(), b.data(), ra[0]))) {
        printf("MISMATCH mode %d at %llu: rc %d / %d, out_len %llu / %llu, rule %llu / %llu\n", mode, (unsigned long long)v, rca, rcb, (unsigned long long)ra[0],
               (unsigned long long)rb[0], (unsigned long long)ra[2], (unsigned long long)rb[2]);
        return 1;
      }
      checked++; forked += f3[2];
    }
  }
  printf("trained_check ok rc %d out_len %llu checked %llu forked %llu\n", rca, (unsigned long long)ra[0], (unsigned long long)checked, (unsigned long long)forked);
  return 0;
}
#endif
