// zada_sizing.h -- how many atoms the entropy workspace is booked for (host only; g++ compiles it for tests/hostcheck).
//
// The invariant: what deflate_spans books before the first span is at least what range_open asks for on ANY span of
// the stream -- any length up to the span, any number of carried atoms below a flush + 1.  ensure_entropy_workspace frees the atom
// arrays when it books anew, and between two spans the carried atoms and their look-behind live in them: a request that exceeds
// the booking in mid stream loses them.  tests/test_hostlogic.py checks the invariant over every span size and "atoms_pct".
#pragma once
#include <stdint.h>

namespace zada {

constexpr uint64_t SIZING_FLUSH = 65536;          // atoms per flush (== FLUSH, zada_internal.h): a span carries fewer than this
constexpr uint64_t SIZING_MIB = 1ull << 20;
constexpr uint64_t SIZING_EXACT_BELOW = 4ull << 20;   // ranges shorter than this are booked at one atom per byte

struct EntropyRequest { uint64_t atoms, out_bytes; };            // what a caller asks ensure_entropy_workspace for
struct EntropyRoom { uint64_t cap_atoms, out_need, cap_out; };   // what that request needs / what a booking for it provides

inline uint64_t sizing_pct(int knob_atoms_pct) { return knob_atoms_pct < 1 ? 1 : knob_atoms_pct > 100 ? 100 : (uint64_t)knob_atoms_pct; }

// The guess for a range of n bytes: "atoms_pct" atoms per 100 bytes and 1 MiB, never more than one atom per byte.
inline uint64_t sizing_guess(uint64_t n, uint64_t pct) {
  const uint64_t guess = n < SIZING_EXACT_BELOW ? n : n / 100 * pct + SIZING_MIB;
  return guess < n ? guess : n;
}

// range_open: the guess for its n bytes and the atoms carried over from the span before.
inline EntropyRequest sizing_range_request(uint64_t n, uint64_t pct, uint64_t carry_atoms) {
  return EntropyRequest{sizing_guess(n, pct) + carry_atoms, n};
}

// deflate_spans: the largest request any range_open of the stream can make.  sizing_guess is not monotone in n (it steps down
// at 4 MiB, where the percentage takes over from one atom per byte), so the maximum over n <= span is taken at the span itself
// or just below the step, whichever is the larger; the carry is at most a flush (FLUSH - 1 atoms and the one range_open adds).
inline EntropyRequest sizing_span_booking(uint64_t span, uint64_t pct) {
  uint64_t atoms = sizing_guess(span, pct);
  if (span >= SIZING_EXACT_BELOW && atoms < SIZING_EXACT_BELOW - 1) atoms = SIZING_EXACT_BELOW - 1;
  return EntropyRequest{atoms + SIZING_FLUSH + 4096, span + SIZING_FLUSH + 4096};
}

// ensure_entropy_workspace: the room a request needs (it books anew when it has less) and the room a booking made for it has.
inline EntropyRoom sizing_entropy_room(EntropyRequest q) {
  if (q.out_bytes < q.atoms) q.out_bytes = q.atoms;
  EntropyRoom r;
  r.out_need = q.out_bytes + q.out_bytes / 8 + SIZING_MIB;
  r.cap_atoms = ((q.atoms < SIZING_MIB ? SIZING_MIB : q.atoms) + 65535) & ~65535ull;
  // the largest stream the encoder can produce for that many bytes: every literal in nine bits (fixed code) + block overheads
  const uint64_t ob = ((q.out_bytes < SIZING_MIB ? SIZING_MIB : q.out_bytes) + 65535) & ~65535ull;
  r.cap_out = ob + ob / 8 + SIZING_MIB;
  return r;
}

}  // namespace zada
