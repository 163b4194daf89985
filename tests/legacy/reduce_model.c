/* CPU model of Reduce_1 .. Reduce_4 (Zip formats 2 .. 5): an LZSS matcher over a binary search tree (4 096-byte ring, look-ahead 31 / 63 /
 * 255 / 191 by factor, threshold 3) whose tokens are written as raw bytes with the escape 144, in front of a per-stream follower-set coder.
 *
 *   reduce_stated : the encoder as the reference states it -- two passes of the matcher, the first one counting byte pairs and filling a
 *                   256 KiB ring cache of raw bytes, the second one leaving the matcher ("derail") as soon as the cache holds the rest; rows
 *                   ordered by a bubble sort that swaps on "<" only; the sizes compared in floating point.
 *   reduce_closed : the form the GPU kernels use (csrc/zada_reduce.hip) -- one pass of the matcher into a raw buffer, rows ordered by a stable
 *                   rank (larger count first, smaller symbol first among equals), sizes compared in integers.
 *   reduce_decode : a decoder written from APPNOTE 5.2.
 *
 * Both encoders return the stream, the raw bytes, Slen and the followers, and fill a census (REDUCE_CENSUS values).
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

enum { N = 4096, THR = 3, NIL = N, DLE = 144, CACHE = 1 << 18 };
enum { C_LIT144, C_EXPANDED, C_TWO_BYTE, C_SLEN0, C_SLEN2, C_SLEN4, C_SLEN8, C_SLEN16, C_SLEN32, REDUCE_CENSUS };
static const int LOOK[5] = {0, 31, 63, 255, 191};
static int b_table(int x) { int b = 1; if (x == 0) return 8; while ((1 << b) < x) b++; return b; }   /* bits of (x - 1) mod 256 */

/* ------------------------------------------------------------------ the matcher (both forms) */
typedef struct Lz Lz;
struct Lz {
  int F;
  uint16_t lson[N + 1], dad[N + 1], rson[N + 257];
  uint8_t text[N + 255];
  int mpos, mlen;
  void (*literal)(void *, uint8_t);
  void (*pair)(void *, int, int);
  int *stop;                                           /* set by the writer when the second pass leaves the matcher */
  void *user;
};
static void lz_insert(Lz *z, int r) {
  const int F = z->F;
  int p = N + 1 + z->text[r], geq = 1;
  z->rson[r] = z->lson[r] = NIL;
  z->mlen = 0;
  for (;;) {
    uint16_t *son = geq ? z->rson : z->lson;
    if (son[p] == NIL) { son[p] = (uint16_t)r; z->dad[r] = (uint16_t)p; return; }
    p = son[p];
    int i = 1;
    while (i < F && z->text[r + i] == z->text[p + i]) i++;
    geq = i == F || z->text[r + i] >= z->text[p + i];
    if (i > THR) {
      const int c = ((r - p) & (N - 1)) - 1;
      if (i > z->mlen) { z->mpos = c; z->mlen = i; if (i >= F) break; }
      else if (i == z->mlen && c < z->mpos) z->mpos = c;
    }
  }
  /* a match of the whole look-ahead: r takes p's place in the tree */
  z->dad[r] = z->dad[p]; z->lson[r] = z->lson[p]; z->rson[r] = z->rson[p];
  z->dad[z->lson[p]] = (uint16_t)r; z->dad[z->rson[p]] = (uint16_t)r;
  if (z->rson[z->dad[p]] == p) z->rson[z->dad[p]] = (uint16_t)r; else z->lson[z->dad[p]] = (uint16_t)r;
  z->dad[p] = NIL;
}
static void lz_delete(Lz *z, int p) {
  int q;
  if (z->dad[p] == NIL) return;
  if (z->rson[p] == NIL) q = z->lson[p];
  else if (z->lson[p] == NIL) q = z->rson[p];
  else {
    q = z->lson[p];
    if (z->rson[q] != NIL) {
      do q = z->rson[q]; while (z->rson[q] != NIL);
      z->rson[z->dad[q]] = z->lson[q]; z->dad[z->lson[q]] = z->dad[q];
      z->lson[q] = z->lson[p]; z->dad[z->lson[p]] = (uint16_t)q;
    }
    z->rson[q] = z->rson[p]; z->dad[z->rson[p]] = (uint16_t)q;
  }
  z->dad[q] = z->dad[p];
  if (z->rson[z->dad[p]] == p) z->rson[z->dad[p]] = (uint16_t)q; else z->lson[z->dad[p]] = (uint16_t)q;
  z->dad[p] = NIL;
}
static void lz_run(Lz *z, int factor, const uint8_t *in, uint64_t n) {
  const int F = LOOK[factor];
  uint64_t pos = 0;
  if (n == 0) return;
  z->F = F;
  for (int i = N + 1; i < N + 257; i++) z->rson[i] = NIL;
  for (int i = 0; i < N; i++) z->dad[i] = NIL;
  memset(z->text, ' ', sizeof z->text);
  int s = 0, r = N - F, len = 0;
  while (len < F && pos < n) z->text[r + len++] = in[pos++];
  lz_insert(z, r);
  do {
    if (z->mlen > len) z->mlen = len;
    if (z->mlen <= THR) { z->mlen = 1; z->literal(z->user, z->text[r]); }
    else z->pair(z->user, z->mpos + 1, z->mlen);
    if (*z->stop) return;
    const int last = z->mlen;
    int i = 0;
    while (i < last && pos < n) {
      i++;
      lz_delete(z, s);
      const uint8_t c = in[pos++];
      z->text[s] = c;
      if (s < F - 1) z->text[s + N] = c;
      s = (s + 1) & (N - 1); r = (r + 1) & (N - 1);
      lz_insert(z, r);
    }
    while (i < last) {
      i++;
      lz_delete(z, s);
      s = (s + 1) & (N - 1); r = (r + 1) & (N - 1);
      if (--len > 0) lz_insert(z, r);
    }
  } while (len > 0);
}

/* ------------------------------------------------------------------ the writer of raw bytes and of the stream */
typedef struct {
  int factor, phase;                                   /* phase 0: statistics, 1: the stream */
  uint8_t ring[N]; int R;                              /* Reduce's own text ring */
  uint32_t markov[256][256];
  uint8_t slen[256], foll[256][32], has[256][256], fpos[256][256];
  int last_b;
  /* the stated form's cache */
  uint8_t *cache; uint32_t cache_nxt; uint64_t cache_cnt, lz_pos, lz_size;
  int use_cache, using_lz, stop;
  /* raw bytes as they pass through the stream phase (stated) or the only pass (closed) */
  uint8_t *raw; uint64_t raw_cap, raw_len;
  /* bit writer */
  uint8_t *out; uint64_t cap, len; uint32_t save; int used;
  uint64_t *cs;
} Wr;

static void put_code(Wr *w, uint32_t code, int size) {
  for (int k = 0; k < size; k++) {
    w->save |= ((code >> k) & 1u) << w->used;
    if (++w->used == 8) { if (w->len < w->cap) w->out[w->len] = (uint8_t)w->save; w->len++; w->save = 0; w->used = 0; }
  }
}
static void code_raw(Wr *w, uint8_t b) {
  if (w->slen[w->last_b] == 0) put_code(w, b, 8);
  else if (w->has[w->last_b][b]) { put_code(w, 0, 1); put_code(w, w->fpos[w->last_b][b], b_table(w->slen[w->last_b])); }
  else { put_code(w, 1, 1); put_code(w, b, 8); }
}
static void raw_byte(Wr *w, uint8_t b) {
  if (w->stop) return;
  w->lz_pos++;
  if (w->phase == 0) {
    w->markov[w->last_b][b]++;
    if (w->use_cache) {
      w->cache[w->cache_nxt] = b; w->cache_nxt = (w->cache_nxt + 1) & (CACHE - 1);
      if (w->cache_cnt < CACHE) w->cache_cnt++;
    }
    if (!w->use_cache) { if (w->raw_len < w->raw_cap) w->raw[w->raw_len] = b; w->raw_len++; }
  } else {
    code_raw(w, b);
    if (w->raw_len < w->raw_cap) w->raw[w->raw_len] = b;
    w->raw_len++;
  }
  w->last_b = b;
  if (w->phase == 1 && w->using_lz && w->lz_size - w->lz_pos < w->cache_cnt) w->stop = 1;   /* the cache holds the rest */
}
static void wr_literal(void *u, uint8_t b) {
  Wr *w = (Wr *)u;
  raw_byte(w, b);
  if (b == DLE) { raw_byte(w, 0); if (w->phase == 0) w->cs[C_LIT144]++; }
  w->ring[w->R] = b; w->R = (w->R + 1) & (N - 1);
}
static void wr_pair(void *u, int distance, int length) {
  Wr *w = (Wr *)u;
  const int f = w->factor, start = (w->R - distance) & (N - 1), len = length - 3, dis = distance - 1;
  const int shift = 1 << (8 - f), max1 = shift - 1;
  if (distance >= 1 && distance <= (1 << f) * 256 && length >= 4 && length <= shift + 257) {
    raw_byte(w, DLE);
    const int upper = (dis / 256) * shift;
    if (len < max1) raw_byte(w, (uint8_t)(len + upper));
    else { raw_byte(w, (uint8_t)(max1 + upper)); raw_byte(w, (uint8_t)(len - max1)); if (w->phase == 0) w->cs[C_TWO_BYTE]++; }
    raw_byte(w, (uint8_t)(dis & 255));
    for (int k = 0; k < length; k++) { w->ring[w->R] = w->ring[(start + k) & (N - 1)]; w->R = (w->R + 1) & (N - 1); }
  } else {
    if (w->phase == 0) w->cs[C_EXPANDED]++;
    for (int k = 0; k < length; k++) wr_literal(w, w->ring[(start + k) & (N - 1)]);
  }
}
static void wr_pass(Wr *w, Lz *z, const uint8_t *in, uint64_t n) {
  memset(w->ring, 0, sizeof w->ring);                  /* (never read before it is written) */
  w->R = N - LOOK[w->factor];
  w->last_b = 0; w->stop = 0; w->using_lz = 1;
  z->literal = wr_literal; z->pair = wr_pair; z->stop = &w->stop; z->user = w;
  lz_run(z, w->factor, in, n);
}
static void save_followers(Wr *w) {
  for (int x = 255; x >= 0; x--) {
    put_code(w, w->slen[x], 6);
    for (int i = 0; i < w->slen[x]; i++) put_code(w, w->foll[x][i], 8);
  }
}
static const int MAX_FOLLO[6] = {-1, 1, 3, 7, 15, 31};
static void census_rows(Wr *w) {
  for (int x = 0; x < 256; x++) { const int s = w->slen[x]; w->cs[s == 0 ? C_SLEN0 : s == 2 ? C_SLEN2 : s == 4 ? C_SLEN4 : s == 8 ? C_SLEN8 : s == 16 ? C_SLEN16 : C_SLEN32]++; }
}

static void followers_stated(Wr *w) {
  static uint8_t order[256];
  memset(w->has, 0, sizeof w->has);
  for (int si = 0; si < 256; si++) {
    uint32_t *row = w->markov[si], total = 0, cum_bl[6] = {0, 0, 0, 0, 0, 0}, cumul = 0;
    for (int sj = 0; sj < 256; sj++) { order[sj] = (uint8_t)sj; total += row[sj]; }
    for (int left = 0;; left++) {                      /* the bubble sort: larger counts towards the front, swapping on "<" only */
      int swapped = 0;
      for (int i = 254; i >= left; i--)
        if (row[i] < row[i + 1]) {
          const uint32_t c = row[i]; row[i] = row[i + 1]; row[i + 1] = c;
          const uint8_t o = order[i]; order[i] = order[i + 1]; order[i + 1] = o;
          swapped = 1;
        }
      if (!swapped) break;
    }
    for (int sj = 0; sj < 32; sj++) {
      cumul += row[sj];
      cum_bl[b_table(sj + 1)] = cumul;
      w->foll[si][sj] = order[sj];
      w->fpos[si][order[sj]] = (uint8_t)sj;
    }
    double min_size = (double)total * 8.0;
    int bits_min = 0;
    for (int bits = 1; bits <= 5; bits++) {
      const double exp_size = (double)cum_bl[bits] * (double)(bits + 1) + (double)(total - cum_bl[bits]) * 9.0 + (double)(MAX_FOLLO[bits] + 1) * 8.0;
      if (exp_size < min_size) { min_size = exp_size; bits_min = bits; }
    }
    w->slen[si] = (uint8_t)(MAX_FOLLO[bits_min] + 1);
    for (int sj = 0; sj <= MAX_FOLLO[bits_min]; sj++) w->has[si][w->foll[si][sj]] = 1;
  }
}
static void followers_closed(Wr *w) {
  memset(w->has, 0, sizeof w->has);
  for (int si = 0; si < 256; si++) {
    const uint32_t *row = w->markov[si];
    uint32_t sorted[32];
    uint64_t total = 0, cum[6] = {0, 0, 0, 0, 0, 0}, c = 0;
    memset(sorted, 0, sizeof sorted);
    for (int j = 0; j < 256; j++) total += row[j];
    /* the rank of a symbol: how many come before it -- a larger count first, the smaller symbol first among equals.  The symbols that occur are
       ranked among themselves; the others follow in their own order. */
    int nz[256], nnz = 0, r;
    for (int j = 0; j < 256; j++) if (row[j]) nz[nnz++] = j;
    for (int a = 0; a < nnz; a++) {
      const int j = nz[a];
      int rank = 0;
      for (int b = 0; b < nnz; b++) { const int i = nz[b]; rank += row[i] > row[j] || (row[i] == row[j] && i < j); }
      if (rank < 32) { w->foll[si][rank] = (uint8_t)j; sorted[rank] = row[j]; w->fpos[si][j] = (uint8_t)rank; }
    }
    r = nnz;
    for (int j = 0; j < 256 && r < 32; j++) if (!row[j]) { w->foll[si][r] = (uint8_t)j; w->fpos[si][j] = (uint8_t)r; r++; }
    for (int k = 0; k < 32; k++) { c += sorted[k]; cum[b_table(k + 1)] = c; }
    uint64_t min_size = total * 8;
    int bits_min = 0;
    for (int bits = 1; bits <= 5; bits++) {
      const uint64_t e = cum[bits] * (uint64_t)(bits + 1) + (total - cum[bits]) * 9 + (uint64_t)(MAX_FOLLO[bits] + 1) * 8;
      if (e < min_size) { min_size = e; bits_min = bits; }
    }
    w->slen[si] = (uint8_t)(MAX_FOLLO[bits_min] + 1);
    for (int k = 0; k < w->slen[si]; k++) w->has[si][w->foll[si][k]] = 1;
  }
}

static uint64_t finish(Wr *w, Lz *z, uint64_t *raw_len, uint8_t *slen, uint8_t *foll) {
  if (w->used) { if (w->len < w->cap) w->out[w->len] = (uint8_t)w->save; w->len++; }
  if (raw_len) *raw_len = w->raw_len;
  if (slen) memcpy(slen, w->slen, 256);
  if (foll) memcpy(foll, w->foll, 256 * 32);
  const uint64_t len = w->len;
  free(w->cache); free(w); free(z);
  return len;
}

uint64_t reduce_stated(int factor, const uint8_t *in, uint64_t n, uint8_t *out, uint64_t cap, uint8_t *raw, uint64_t raw_cap, uint64_t *raw_len,
                       uint8_t *slen, uint8_t *foll, uint64_t *census) {
  uint64_t dummy[REDUCE_CENSUS];
  Wr *w = (Wr *)calloc(1, sizeof(Wr));
  Lz *z = (Lz *)calloc(1, sizeof(Lz));
  if (!census) census = dummy;
  memset(census, 0, sizeof(uint64_t) * REDUCE_CENSUS);
  w->factor = factor; w->cs = census; w->out = out; w->cap = cap; w->raw = raw; w->raw_cap = raw_cap;
  w->cache = (uint8_t *)malloc(CACHE); w->use_cache = 1;
  w->phase = 0;                                        /* pass 1: the pair counts, and the cache */
  wr_pass(w, z, in, n);
  followers_stated(w);
  census_rows(w);
  save_followers(w);
  w->lz_size = w->lz_pos; w->lz_pos = 0;
  w->phase = 1;                                        /* pass 2: the stream; the matcher runs until the cache holds the rest */
  wr_pass(w, z, in, n);
  if (w->stop) {
    w->stop = 0; w->using_lz = 0;
    for (uint32_t i = (uint32_t)(w->lz_pos & (CACHE - 1)); w->lz_pos < w->lz_size; i = (i + 1) & (CACHE - 1)) raw_byte(w, w->cache[i]);
  }
  return finish(w, z, raw_len, slen, foll);
}

uint64_t reduce_closed(int factor, const uint8_t *in, uint64_t n, uint8_t *out, uint64_t cap, uint8_t *raw, uint64_t raw_cap, uint64_t *raw_len,
                       uint8_t *slen, uint8_t *foll, uint64_t *census) {
  uint64_t dummy[REDUCE_CENSUS];
  Wr *w = (Wr *)calloc(1, sizeof(Wr));
  Lz *z = (Lz *)calloc(1, sizeof(Lz));
  if (!census) census = dummy;
  memset(census, 0, sizeof(uint64_t) * REDUCE_CENSUS);
  w->factor = factor; w->cs = census; w->out = out; w->cap = cap;
  w->raw_cap = 2 * n + 16; w->raw = (uint8_t *)malloc(w->raw_cap);
  w->phase = 0;
  wr_pass(w, z, in, n);                                /* the only pass of the matcher */
  followers_closed(w);
  census_rows(w);
  save_followers(w);
  w->phase = 1; w->last_b = 0;
  const uint64_t rl = w->raw_len;
  uint8_t *own = w->raw;
  for (uint64_t i = 0; i < rl; i++) { code_raw(w, own[i]); w->last_b = own[i]; }
  if (raw) memcpy(raw, own, rl < raw_cap ? rl : raw_cap);
  free(own);
  w->raw = NULL;
  return finish(w, z, raw_len, slen, foll);
}

/* ------------------------------------------------------------------ the decoder (APPNOTE 5.2) */
int64_t reduce_decode(int factor, const uint8_t *in, uint64_t n_in, uint8_t *out, uint64_t cap) {
  static uint8_t slen[256], foll[256][64];
  const uint64_t nbits = n_in * 8;
  uint64_t bitpos = 0, olen = 0;
#define GET(v, k) do { if (bitpos + (k) > nbits) return -1; uint32_t w_ = 0; for (int j_ = 0; j_ < (k); j_++, bitpos++) w_ |= (uint32_t)((in[bitpos >> 3] >> (bitpos & 7)) & 1) << j_; (v) = (int)w_; } while (0)
  for (int x = 255; x >= 0; x--) {
    int s;
    GET(s, 6);
    slen[x] = (uint8_t)s;
    for (int i = 0; i < s; i++) { int f; GET(f, 8); foll[x][i] = (uint8_t)f; }
  }
  const int lmask = (1 << (8 - factor)) - 1;
  int last = 0, state = 0, v = 0, len = 0;
  while (olen < cap) {
    int c;
    if (slen[last] == 0) GET(c, 8);
    else {
      int flag;
      GET(flag, 1);
      if (flag) GET(c, 8);
      else { int idx; GET(idx, b_table(slen[last])); if (idx >= slen[last]) return -1; c = foll[last][idx]; }
    }
    last = c;
    if (state == 0) { if (c == DLE) state = 1; else out[olen++] = (uint8_t)c; }
    else if (state == 1) {
      if (c == 0) { out[olen++] = DLE; state = 0; }
      else { v = c; len = c & lmask; state = len == lmask ? 2 : 3; }
    } else if (state == 2) { len += c; state = 3; }
    else {
      const uint64_t dist = (uint64_t)(v >> (8 - factor)) * 256 + (uint64_t)c + 1;
      len += 3;
      for (int k = 0; k < len; k++) {
        if (olen >= cap) return -1;
        out[olen] = dist > olen ? 0 : out[olen - dist];
        olen++;
      }
      state = 0;
    }
  }
#undef GET
  return state == 0 ? (int64_t)olen : -1;
}

/* One input through both forms and the decoder: 0 when the stated form equals the closed form in every result and the decoder returns the input. */
int reduce_check_one(int factor, const uint8_t *d, uint64_t n, uint64_t *census_sum) {
  const uint64_t rcap = 2 * n + 16, cap = rcap + rcap / 8 + 8500;
  uint8_t *a = (uint8_t *)malloc(cap), *b = (uint8_t *)malloc(cap), *ra = (uint8_t *)malloc(rcap), *rb = (uint8_t *)malloc(rcap), *back = (uint8_t *)malloc(n + 1);
  uint8_t sa[256], sb[256], fa[256 * 32], fb[256 * 32];
  uint64_t ca[REDUCE_CENSUS], cb[REDUCE_CENSUS], rla = 0, rlb = 0;
  const uint64_t la = reduce_stated(factor, d, n, a, cap, ra, rcap, &rla, sa, fa, ca), lb = reduce_closed(factor, d, n, b, cap, rb, rcap, &rlb, sb, fb, cb);
  int bad = la != lb || la > cap || memcmp(a, b, la) != 0 || rla != rlb || rla > rcap || memcmp(ra, rb, rla) != 0 || memcmp(sa, sb, 256) != 0 ||
            memcmp(ca, cb, sizeof ca) != 0;
  for (int x = 0; x < 256 && !bad; x++) bad = memcmp(fa + 32 * x, fb + 32 * x, sa[x]) != 0;      /* the followers in use */
  if (!bad) bad = reduce_decode(factor, a, la, back, n) != (int64_t)n || memcmp(back, d, n) != 0;
  if (census_sum) for (int k = 0; k < REDUCE_CENSUS; k++) census_sum[k] += ca[k];
  free(a); free(b); free(ra); free(rb); free(back);
  return bad;
}
static uint32_t lcg(uint32_t *s) { *s = *s * 1664525u + 1013904223u; return *s >> 8; }
/* Seeded self-test over `count` small inputs of 0 .. 3 000 bytes, the factor going round: returns how many inputs fail. */
int reduce_selftest(uint32_t seed, int count, uint64_t *census_sum) {
  int bad = 0;
  uint8_t *d = (uint8_t *)malloc(3001);
  for (int t = 0; t < count; t++) {
    uint32_t s = seed + (uint32_t)t * 104729u;
    const uint64_t n = lcg(&s) % 3001;
    const uint32_t alpha = 1 + lcg(&s) % (t % 8 == 0 ? 64 : 5), base = t % 5 == 0 ? 142 : 'a', period = 1 + lcg(&s) % 700;
    for (uint64_t i = 0; i < n; i++) d[i] = (t & 1) && i >= period && lcg(&s) % 16 ? d[i - period] : (uint8_t)(base + lcg(&s) % alpha);
    bad += reduce_check_one(1 + t % 4, d, n, census_sum);
  }
  free(d);
  return bad;
}
