/* unlegacy_model.c -- CPU models for the tests of the Shrink / Reduce / Implode readers (zip-ada_amd/csrc/zada_unlegacy_logic.h):
 *   - the three decoders in the form the reference states them (UnZip.Decompress.Unshrink / Unreduce / Explode): a 32 KiB slide that is flushed
 *     when full, Copy_or_zero with its `unflushed` flag, Unshrink's free list kept in the negative values of Previous_Code, Explode's codes looked
 *     up in multi-level tables indexed by inverted bits.  They carry the two departures of the logic header (a code that needs a byte beyond n_in;
 *     a string or copy that would pass cap) and nothing else, and they count the branches a stream reaches (the census);
 *   - a small imploder, for test inputs only: a greedy hash matcher, code lengths limited to 16 bits, the tree encodings, all four flag
 *     combinations, and on request a first copy that reaches in front of the entry's start where the data begins with zero bytes.
 * None of this is product code. */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

enum { R_OK = 0, R_INPUT_END = 1, R_OUTPUT_FULL, R_SH_FIRST, R_SH_SIZE, R_SH_SPECIAL, R_SH_STACK, R_IM_RUNS, R_IM_TREE, R_MODEL = 99 };
/* the census, by index */
enum { C_SH_CLEARS = 0, C_SH_RISES, C_SH_ORPHAN_FIRST, C_SH_ORPHAN_LINKED, C_SH_FULL,
       C_RD_LIT144, C_RD_TWO_BYTE, C_RD_B1, C_RD_B2, C_RD_B3, C_RD_B4, C_RD_B5, C_RD_B6, C_RD_B8, C_RD_ZERO_FILL, C_RD_OVERLAP,
       C_IM_EXTRA_LEN, C_IM_ZERO_FILL, C_IM_OVERLAP, C_IM_DIST_4096, C_IM_DIST_8192, C_IM_BEYOND_32K, C_COUNT };

/* ---- Bit_buffer: least significant bit first; a byte beyond the input reads 0 and is counted (departure 1 is judged from the count) ---- */
typedef struct { const uint8_t *in; uint64_t n, ip; uint32_t B; int K; } Bits;
static uint32_t read_byte(Bits *b) { uint32_t v = b->ip < b->n ? b->in[b->ip] : 0u; b->ip++; return v; }
static void need(Bits *b, int n) { while (b->K < n) { b->B |= read_byte(b) << b->K; b->K += 8; } }
static void dump(Bits *b, int n) { b->B >>= n; b->K -= n; }
static uint32_t read_and_dump(Bits *b, int n) { uint32_t v; need(b, n); v = b->B & ((1u << n) - 1u); dump(b, n); return v; }
static uint32_t read_inverted(Bits *b, int n) { need(b, n); return ~b->B & ((1u << n) - 1u); }
static int over(const Bits *b) { return b->ip * 8 - (uint64_t)b->K > b->n * 8; }
static uint64_t used(const Bits *b) { return (b->ip * 8 - (uint64_t)b->K + 7) / 8; }

typedef struct { uint64_t out_len, in_used, rule, in_pos, out_pos; } Res;
static int fail(Res *r, const Bits *b, int rule, uint64_t out_pos) {
  r->out_len = 0; r->in_used = 0; r->rule = (uint64_t)rule; r->in_pos = rule == R_INPUT_END ? b->n : used(b); r->out_pos = out_pos;
  return -7;
}
static int done(Res *r, const Bits *b, uint64_t out_len) {
  r->out_len = out_len; r->in_used = used(b); r->rule = 0; r->in_pos = r->in_used; r->out_pos = out_len;
  return 0;
}

/* ---- the slide ---- */
#define WSIZE 32768
typedef struct { uint8_t slide[WSIZE]; int W; int unflushed; uint8_t *out; uint64_t cap, op; int bad; } Slide;
static void flush(Slide *s, int x) {
  for (int i = 0; i < x; i++) { if (s->op < s->cap) s->out[s->op] = s->slide[i]; else s->bad = 1; s->op++; }
}
static void flush_if_full(Slide *s) { if (s->W == WSIZE) { flush(s, WSIZE); s->W = 0; s->unflushed = 0; } }
static void out_byte(Slide *s, uint32_t b) { s->slide[s->W++] = (uint8_t)b; flush_if_full(s); }
/* a source in front of the first byte of a slide never flushed reads 0; returns what it met: 1 zero-fill, 2 overlap */
static int copy_or_zero(Slide *s, int distance, int length) {
  int source = s->W - distance, remain = length, met = 0;
  if (distance < length) met |= 2;
  do {
    int part;
    source = ((source % WSIZE) + WSIZE) % WSIZE;
    part = source > s->W ? WSIZE - source : WSIZE - s->W;
    if (part > remain) part = remain;
    remain -= part;
    if (s->unflushed && s->W <= source) {
      memset(s->slide + s->W, 0, (size_t)part);
      s->W += part; source += part; met |= 1;
    } else {
      for (int k = 0; k < part; k++) s->slide[s->W++] = s->slide[source++];
    }
    flush_if_full(s);
  } while (remain);
  return met;
}

/* ---- Unshrink ---- */
#define FIRST_ENTRY 257
#define MAX_CODE 8192
#define MAX_STACK 8192
static int unshrink(Bits *b, uint8_t *out, uint64_t cap, Res *r, uint64_t *cs) {
  static int32_t previous_code[MAX_CODE + 1];
  static uint8_t stored_literal[MAX_CODE + 1], stack[MAX_STACK + 1];
  uint64_t S = cap, op = 0;
  int code_size = 9, next_free, actual_max_code, incode, new_code, last_incode, stack_ptr = MAX_STACK;
  uint8_t last_outcode;
  for (int i = FIRST_ENTRY; i <= MAX_CODE; i++) previous_code[i] = -(i + 1);
  memset(stored_literal, 0, sizeof stored_literal);
  if (cap == 0) return done(r, b, 0);
  next_free = FIRST_ENTRY; actual_max_code = FIRST_ENTRY - 1;
  incode = (int)read_and_dump(b, code_size);
  if (over(b)) return fail(r, b, R_INPUT_END, 0);
  last_incode = incode;
  if (incode > 255) return fail(r, b, R_SH_FIRST, 0);
  last_outcode = (uint8_t)incode;
  out[op++] = last_outcode; S--;
  while (S > 0) {
    incode = (int)read_and_dump(b, code_size);
    if (over(b)) return fail(r, b, R_INPUT_END, op);
    if (incode == 256) {
      incode = (int)read_and_dump(b, code_size);
      if (over(b)) return fail(r, b, R_INPUT_END, op);
      if (incode == 1) {
        code_size++; cs[C_SH_RISES]++;
        if (code_size > 13) return fail(r, b, R_SH_SIZE, op);
      } else if (incode == 2) {                         /* Clear_Leaf_Nodes */
        static uint8_t is_leaf[MAX_CODE + 1];
        int pc;
        cs[C_SH_CLEARS]++;
        memset(is_leaf, 1, sizeof is_leaf);
        for (int i = FIRST_ENTRY; i <= actual_max_code; i++) { pc = previous_code[i]; if (pc > 256) is_leaf[pc] = 0; }
        pc = -1; next_free = -1;
        for (int i = FIRST_ENTRY; i <= actual_max_code; i++)
          if (previous_code[i] < 0 || is_leaf[i]) {
            if (pc == -1) next_free = i; else previous_code[pc] = -i;
            pc = i;
          }
        if (pc != -1) previous_code[pc] = -(actual_max_code + 1);
        if (next_free == -1) next_free = actual_max_code + 1;
      } else return fail(r, b, R_SH_SPECIAL, op);
      continue;
    }
    new_code = incode;
    if (incode < 256) {
      last_outcode = (uint8_t)incode;
      out[op++] = last_outcode; S--;
    } else {
      uint64_t len;
      if (previous_code[incode] < 0) {                  /* first node is orphan */
        cs[C_SH_ORPHAN_FIRST]++;
        stack[stack_ptr--] = last_outcode;
        incode = last_incode;
      }
      while (incode > 256) {
        if (stack_ptr < 0) return fail(r, b, R_SH_STACK, op);
        if (incode > MAX_CODE) return fail(r, b, R_MODEL, op);
        if (previous_code[incode] < 0) {                /* linked node is orphan */
          cs[C_SH_ORPHAN_LINKED]++;
          stack[stack_ptr] = last_outcode;
          incode = last_incode;
        } else {
          stack[stack_ptr] = stored_literal[incode];
          incode = previous_code[incode];
        }
        stack_ptr--;
      }
      last_outcode = (uint8_t)incode;
      len = (uint64_t)(MAX_STACK - stack_ptr) + 1;
      if (len > S) return fail(r, b, R_OUTPUT_FULL, op);            /* departure 2 */
      out[op++] = last_outcode;
      for (int i = stack_ptr + 1; i <= MAX_STACK; i++) out[op++] = stack[i];
      S -= len;
      stack_ptr = MAX_STACK;
    }
    {                                                    /* Attempt_Table_Increase */
      const int candidate = next_free;
      if (candidate > MAX_CODE) cs[C_SH_FULL]++;
      else {
        if (candidate < FIRST_ENTRY || previous_code[candidate] >= 0) return fail(r, b, R_MODEL, op);
        next_free = -previous_code[candidate];
        if (next_free - 1 > actual_max_code) actual_max_code = next_free - 1;
        previous_code[candidate] = last_incode;
        stored_literal[candidate] = last_outcode;
      }
    }
    last_incode = new_code;
  }
  return done(r, b, op);
}

/* ---- Unreduce ---- */
static int b_table(int x) {
  if (x == 0) return 8;
  if (x <= 2) return 1;
  if (x <= 4) return 2;
  if (x <= 8) return 3;
  if (x <= 16) return 4;
  if (x <= 32) return 5;
  if (x <= 64) return 6;
  if (x <= 128) return 7;
  return 8;
}
static int unreduce(Bits *b, int factor, Slide *s, uint64_t cap, Res *r, uint64_t *cs) {
  static uint8_t followers[256][64];
  uint8_t slen[256];
  uint64_t S = cap;
  int length = 0, char_read, last_char = 0, state = 0;
  uint32_t V = 0;
  const uint32_t max_and = (1u << (8 - factor)) - 1u;
  memset(followers, 0, sizeof followers);
  for (int x = 255; x >= 0; x--) {
    slen[x] = (uint8_t)read_and_dump(b, 6);
    for (int i = 0; i < slen[x]; i++) followers[x][i] = (uint8_t)read_and_dump(b, 8);
    if (over(b)) return fail(r, b, R_INPUT_END, 0);
  }
  while (S > 0) {
    if (slen[last_char] == 0) { char_read = (int)read_and_dump(b, 8); cs[C_RD_B8]++; }
    else if (read_and_dump(b, 1) == 0) {
      const int nb = b_table(slen[last_char]);
      cs[C_RD_B1 + nb - 1]++;
      char_read = followers[last_char][read_and_dump(b, nb)];
    } else { char_read = (int)read_and_dump(b, 8); cs[C_RD_B8]++; }
    if (over(b)) return fail(r, b, R_INPUT_END, cap - S);
    switch (state) {
      case 0:
        if (char_read == 144) state = 1; else { S--; out_byte(s, (uint32_t)char_read); }
        break;
      case 1:
        if (char_read == 0) { S--; out_byte(s, 144); state = 0; cs[C_RD_LIT144]++; }
        else {
          V = (uint32_t)char_read;
          length = (int)(V & max_and);
          state = length == (int)max_and ? 2 : 3;
        }
        break;
      case 2:
        length += char_read; state = 3; cs[C_RD_TWO_BYTE]++;
        break;
      default: {
        int met;
        length += 3;
        if ((uint64_t)length > S) return fail(r, b, R_OUTPUT_FULL, cap - S);     /* departure 2 */
        S -= (uint64_t)length;
        met = copy_or_zero(s, char_read + 1 + (int)((V >> (8 - factor)) << 8), length);
        if (met & 1) cs[C_RD_ZERO_FILL]++;
        if (met & 2) cs[C_RD_OVERLAP]++;
        state = 0;
      }
    }
    last_char = char_read;
  }
  flush(s, s->W);
  return done(r, b, cap);
}

/* ---- Explode: multi-level tables indexed by the stream's bits, inverted ---- */
enum { E_INVALID = 99 };
typedef struct HT { uint8_t e, b; uint16_t n; struct HT *next; } HT;
static HT *ht_pool[64];
static int ht_pools;
static void ht_free_all(void) { while (ht_pools) free(ht_pool[--ht_pools]); }
static uint32_t rev(uint32_t c, int len) { uint32_t v = 0; for (int i = 0; i < len; i++) v |= ((c >> i) & 1u) << (len - 1 - i); return v; }
/* the table behind `w` bits equal to `prefix` (as the stream gives them, inverted): *width receives its index width */
static HT *ht_level(const uint8_t *len, const uint16_t *rcode, int N, int w, uint32_t prefix, int m, int s, const uint16_t *d, const uint8_t *e, int *width) {
  int longest = 0, j;
  HT *t;
  for (int v = 0; v < N; v++) if (len[v] > w && (rcode[v] & ((1u << w) - 1u)) == prefix && len[v] > longest) longest = len[v];
  j = longest - w < m ? longest - w : m;
  if (w == 0) j = m;                                    /* the main table always has m bits */
  if (ht_pools == 64) return NULL;
  t = (HT *)malloc(sizeof(HT) << j);
  if (!t) return NULL;
  ht_pool[ht_pools++] = t;
  for (int k = 0; k < 1 << j; k++) { t[k].e = E_INVALID; t[k].b = 0; t[k].n = 0; t[k].next = NULL; }
  for (int v = 0; v < N; v++) {
    uint32_t idx;
    if (len[v] <= w || (rcode[v] & ((1u << w) - 1u)) != prefix) continue;
    idx = (rcode[v] >> w) & ((1u << j) - 1u);
    if (len[v] - w <= j) {
      for (uint32_t k = idx; k < 1u << j; k += 1u << (len[v] - w)) {
        t[k].b = (uint8_t)(len[v] - w);
        if (v < s) { t[k].e = 16; t[k].n = (uint16_t)v; } else { t[k].e = e[v - s]; t[k].n = d[v - s]; }
      }
    } else if (!t[idx].next) {
      int sub = 0;
      t[idx].next = ht_level(len, rcode, N, w + j, prefix | idx << w, m, s, d, e, &sub);
      if (!t[idx].next) return NULL;
      t[idx].b = (uint8_t)j;
      t[idx].e = (uint8_t)(16 + sub);
    }
  }
  *width = j;
  return t;
}
/* 0, or R_IM_TREE for lengths over-subscribed or incomplete; *m: in, the width asked for; out, the main table's */
static int huft_build(const uint8_t *len, int N, int s, const uint16_t *d, const uint8_t *e, HT **t, int *m) {
  int count[17] = {0}, lo = 1, hi = 16, y, width = 0;
  uint16_t rcode[256], next[17];
  for (int v = 0; v < N; v++) count[len[v]]++;
  while (lo <= 16 && !count[lo]) lo++;
  while (hi > 0 && !count[hi]) hi--;
  if (*m < lo) *m = lo;
  if (*m > hi) *m = hi;
  y = 1 << lo;
  for (int j = lo; j < hi; j++) { y -= count[j]; if (y < 0) return R_IM_TREE; y *= 2; }
  y -= count[hi];
  if (y < 0) return R_IM_TREE;
  if (y != 0 && hi != 1) return R_IM_TREE;              /* huft_incomplete */
  { uint32_t c = 0; for (int l = 1; l <= 16; l++) { c = (c + (uint32_t)count[l - 1]) << 1; next[l] = (uint16_t)c; } }
  for (int v = 0; v < N; v++) rcode[v] = (uint16_t)rev(next[len[v]]++, len[v]);
  *t = ht_level(len, rcode, N, 0, 0, *m, s, d, e, &width);
  return *t ? 0 : R_MODEL;
}
static int get_tree(Bits *b, uint8_t *L, uint32_t N) {
  uint32_t I = read_byte(b) + 1, K = 0;
  if (b->ip > b->n) return R_INPUT_END;
  do {
    uint32_t J = read_byte(b), Bl;
    if (b->ip > b->n) return R_INPUT_END;
    Bl = (J & 15) + 1;
    J = (J >> 4) + 1;
    if (K + J > N) return R_IM_RUNS;
    do { L[K++] = (uint8_t)Bl; } while (--J);
  } while (--I);
  return K != N ? R_IM_RUNS : 0;
}
/* the lookup loop of Explode_Lit / Explode_Nolit; -1: an invalid entry */
static int lookup(Bits *b, const HT *t, int bits, int *e_out) {
  uint32_t ci = read_inverted(b, bits);
  int e;
  for (;;) {
    e = t[ci].e;
    if (e <= 16) break;
    if (e == E_INVALID) return -1;
    dump(b, t[ci].b);
    e -= 16;
    t = t[ci].next;
    ci = read_inverted(b, e);
  }
  dump(b, t[ci].b);
  *e_out = e;
  return t[ci].n;
}
static int explode(Bits *b, int flags, Slide *s, uint64_t cap, Res *r, uint64_t *cs) {
  uint8_t L[256], extra[64];
  uint16_t cp_len[64], cp_dist[64];
  const int lit_tree = (flags & 4) != 0, big = (flags & 2) != 0, needed = big ? 7 : 6;
  HT *Tb = NULL, *Tl = NULL, *Td = NULL;
  int Bb = 9, Bl = 7, Bd = b->n > 200000 ? 8 : 7, rule = 0;
  uint64_t S = cap;
  for (int i = 0; i < 64; i++) { extra[i] = i == 63 ? 8 : 0; cp_len[i] = (uint16_t)(i + (lit_tree ? 3 : 2)); cp_dist[i] = (uint16_t)(1 + i * (big ? 128 : 64)); }
  if (lit_tree) { rule = get_tree(b, L, 256); if (!rule) rule = huft_build(L, 256, 256, NULL, NULL, &Tb, &Bb); }
  if (!rule) rule = get_tree(b, L, 64);
  if (!rule) rule = huft_build(L, 64, 0, cp_len, extra, &Tl, &Bl);
  if (!rule) rule = get_tree(b, L, 64);
  if (!rule) rule = huft_build(L, 64, 0, cp_dist, extra, &Td, &Bd);
  if (rule) { ht_free_all(); return fail(r, b, rule, 0); }
  b->B = 0; b->K = 0;
  while (S > 0) {
    int e, n, d;
    if (read_and_dump(b, 1)) {
      int c = lit_tree ? lookup(b, Tb, Bb, &e) : (int)read_and_dump(b, 8);
      if (c < 0) { ht_free_all(); return fail(r, b, R_MODEL, cap - S); }
      if (over(b)) { ht_free_all(); return fail(r, b, R_INPUT_END, cap - S); }
      S--;
      out_byte(s, (uint32_t)c);
    } else {
      int met, dd;
      d = (int)read_and_dump(b, needed);
      dd = lookup(b, Td, Bd, &e);
      n = lookup(b, Tl, Bl, &e);
      if (dd < 0 || n < 0) { ht_free_all(); return fail(r, b, R_MODEL, cap - S); }
      d += dd;
      if (e) { n += (int)read_and_dump(b, 8); cs[C_IM_EXTRA_LEN]++; }
      if (over(b)) { ht_free_all(); return fail(r, b, R_INPUT_END, cap - S); }
      if ((uint64_t)n > S) { ht_free_all(); return fail(r, b, R_OUTPUT_FULL, cap - S); }     /* departure 2 */
      S -= (uint64_t)n;
      met = copy_or_zero(s, d, n);
      if (met & 1) cs[C_IM_ZERO_FILL]++;
      if (met & 2) cs[C_IM_OVERLAP]++;
      if (d == 4096) cs[C_IM_DIST_4096]++;
      if (d == 8192) cs[C_IM_DIST_8192]++;
    }
  }
  if (cap > WSIZE) cs[C_IM_BEYOND_32K]++;
  flush(s, s->W);
  ht_free_all();
  return done(r, b, cap);
}

/* returns 0, -7 (the stream is not valid) or -1 (method); res5 = out_len, in_used, rule, input byte, output position; census [C_COUNT] is added
 * to; out (cap bytes) holds out_len bytes where the stream is valid */
int um_decode(int method, int flags, const uint8_t *in, uint64_t n_in, uint8_t *out, uint64_t cap, uint64_t *res5, uint64_t *census) {
  Bits b = {in, n_in, 0, 0, 0};
  Res r;
  int rc;
  if (method < 1 || method > 6) return -1;
  if (method == 1) rc = unshrink(&b, out, cap, &r, census);
  else {
    Slide *s = (Slide *)calloc(1, sizeof(Slide));
    if (!s) return -2;
    s->unflushed = 1; s->out = out; s->cap = cap;
    rc = method == 6 ? explode(&b, flags, s, cap, &r, census) : unreduce(&b, method - 1, s, cap, &r, census);
    if (s->bad || (rc == 0 && s->op != cap)) { rc = -7; r.rule = R_MODEL; }
    free(s);
  }
  res5[0] = r.out_len; res5[1] = r.in_used; res5[2] = r.rule; res5[3] = r.in_pos; res5[4] = r.out_pos;
  return rc;
}
int um_census_count(void) { return C_COUNT; }

/* ---- the imploder (test inputs only) ---- */
typedef struct { uint8_t *p; uint64_t cap, n; uint32_t acc; int k; } Out;
static void put_bits(Out *o, uint32_t v, int n) {
  for (int i = 0; i < n; i++) {
    o->acc |= ((v >> i) & 1u) << o->k;
    if (++o->k == 8) { if (o->n < o->cap) o->p[o->n] = (uint8_t)o->acc; o->n++; o->acc = 0; o->k = 0; }
  }
}
/* a code as Explode reads it: first the most significant bit, every bit inverted */
static void put_code(Out *o, uint32_t code, int len) { for (int i = len - 1; i >= 0; i--) put_bits(o, ~(code >> i) & 1u, 1); }
/* Huffman lengths of N symbols, every one of them coded, none longer than 16 bits */
static void code_lengths(const uint32_t *freq, int N, uint8_t *len) {
  uint32_t f[256];
  for (int v = 0; v < N; v++) f[v] = freq[v] + 1;
  for (;;) {
    uint64_t w[512];
    int parent[512], alive[512], nodes = N, left = N, deepest = 0;
    for (int v = 0; v < N; v++) { w[v] = f[v]; alive[v] = 1; parent[v] = -1; }
    while (left > 1) {
      int a = -1, c = -1;
      for (int v = 0; v < nodes; v++) if (alive[v]) { if (a < 0 || w[v] < w[a]) { c = a; a = v; } else if (c < 0 || w[v] < w[c]) c = v; }
      alive[a] = alive[c] = 0; parent[a] = parent[c] = nodes;
      w[nodes] = w[a] + w[c]; alive[nodes] = 1; parent[nodes] = -1; nodes++; left--;
    }
    for (int v = 0; v < N; v++) { int l = 0; for (int p = v; parent[p] >= 0; p = parent[p]) l++; len[v] = (uint8_t)(l ? l : 1); if (l > deepest) deepest = l; }
    if (deepest <= 16) return;
    for (int v = 0; v < N; v++) f[v] = f[v] / 2 + 1;
  }
}
static void canonical(const uint8_t *len, int N, uint16_t *code) {
  int count[17] = {0};
  uint32_t c = 0, next[17];
  for (int v = 0; v < N; v++) count[len[v]]++;
  for (int l = 1; l <= 16; l++) { c = (c + (uint32_t)count[l - 1]) << 1; next[l] = c; }
  for (int v = 0; v < N; v++) code[v] = (uint16_t)next[len[v]]++;
}
static void put_tree(Out *o, const uint8_t *len, int N) {
  uint8_t runs[256];
  int nr = 0;
  for (int v = 0; v < N;) {
    int k = 1;
    while (v + k < N && len[v + k] == len[v] && k < 16) k++;
    runs[nr++] = (uint8_t)((k - 1) << 4 | (len[v] - 1));
    v += k;
  }
  put_bits(o, (uint32_t)(nr - 1), 8);
  for (int i = 0; i < nr; i++) put_bits(o, runs[i], 8);
}
/* data -> an Implode payload under `flags` (bit 1: 8 KiB, bit 2: three trees); zero_reach > 0: where the data begins with at least the
 * minimum match of zero bytes, the first token is a copy of them from distance zero_reach, i.e. from in front of the entry.  Returns the
 * payload's length (more than cap_out: it did not fit). */
uint64_t um_implode(const uint8_t *data, uint64_t n, int flags, int zero_reach, uint8_t *out, uint64_t cap_out) {
  const int lit_tree = (flags & 4) != 0, low = (flags & 2) ? 7 : 6, min_match = lit_tree ? 3 : 2;
  const uint32_t max_dist = (flags & 2) ? 8192 : 4096, max_len = (uint32_t)min_match + 63 + 255;
  uint32_t *tok = (uint32_t *)malloc((size_t)(n + 1) * 4);              /* literal: byte; copy: 1 << 31 | dist - 1 << 16 | len */
  int32_t *head = (int32_t *)malloc(65536 * 4), *prev = (int32_t *)malloc((size_t)(n + 1) * 4);
  uint32_t flit[256] = {0}, flen[64] = {0}, fdist[64] = {0};
  uint8_t llit[256], llen[64], ldist[64];
  uint16_t clit[256], clen[64], cdist[64];
  uint64_t nt = 0, i = 0;
  Out o = {out, cap_out, 0, 0, 0};
  if (!tok || !head || !prev) { free(tok); free(head); free(prev); return ~0ull; }
  for (int k = 0; k < 65536; k++) head[k] = -1;
  if (zero_reach > 0 && (uint32_t)zero_reach <= max_dist) {
    uint32_t z = 0;
    while (z < n && z < max_len && data[z] == 0) z++;
    if (z >= (uint32_t)min_match) { tok[nt++] = 1u << 31 | (uint32_t)(zero_reach - 1) << 16 | z; i = z; }
  }
  for (uint64_t p = 0; p < i; p++) if (p + 2 <= n) { uint32_t h = (uint32_t)(data[p] | data[p + 1 < n ? p + 1 : p] << 8); prev[p] = head[h]; head[h] = (int32_t)p; }
  while (i < n) {
    uint32_t best = 0, bdist = 0;
    if (i + 2 <= n) {
      const uint32_t h = (uint32_t)(data[i] | data[i + 1] << 8);
      int tries = 256;
      for (int32_t c = head[h]; c >= 0 && i - (uint64_t)c <= max_dist && tries--; c = prev[c]) {
        uint32_t l = 0;
        while (l < max_len && i + l < n && data[(uint64_t)c + l] == data[i + l]) l++;
        if (l > best) { best = l; bdist = (uint32_t)(i - (uint64_t)c); }
      }
    }
    if (best >= (uint32_t)min_match) tok[nt++] = 1u << 31 | (bdist - 1) << 16 | best;
    else { best = 1; tok[nt++] = data[i]; }
    for (uint32_t k = 0; k < best; k++, i++)
      if (i + 2 <= n) { const uint32_t h = (uint32_t)(data[i] | data[i + 1] << 8); prev[i] = head[h]; head[h] = (int32_t)i; }
  }
  for (uint64_t t = 0; t < nt; t++) {
    if (tok[t] >> 31) {
      const uint32_t d = (tok[t] >> 16) & 0x7FFF, l = (tok[t] & 0xFFFF) - (uint32_t)min_match;
      fdist[d >> low]++; flen[l < 63 ? l : 63]++;
    } else flit[tok[t]]++;
  }
  code_lengths(flit, 256, llit); code_lengths(flen, 64, llen); code_lengths(fdist, 64, ldist);
  canonical(llit, 256, clit); canonical(llen, 64, clen); canonical(ldist, 64, cdist);
  if (lit_tree) put_tree(&o, llit, 256);
  put_tree(&o, llen, 64);
  put_tree(&o, ldist, 64);
  for (uint64_t t = 0; t < nt; t++) {
    if (tok[t] >> 31) {
      const uint32_t d = (tok[t] >> 16) & 0x7FFF, l = (tok[t] & 0xFFFF) - (uint32_t)min_match;
      put_bits(&o, 0, 1);
      put_bits(&o, d & ((1u << low) - 1u), low);
      put_code(&o, cdist[d >> low], ldist[d >> low]);
      put_code(&o, clen[l < 63 ? l : 63], llen[l < 63 ? l : 63]);
      if (l >= 63) put_bits(&o, l - 63, 8);
    } else {
      put_bits(&o, 1, 1);
      if (lit_tree) put_code(&o, clit[tok[t]], llit[tok[t]]); else put_bits(&o, tok[t], 8);
    }
  }
  if (o.k) put_bits(&o, 0, 8 - o.k);
  free(tok); free(head); free(prev);
  return o.n;
}
