/* CPU model of Shrink_1 (Zip format 1: LZW with partial clearing, codes of 9 .. 13 bits).
 *
 *   shrink_stated : the encoder as the reference states it -- a code table of child / sibling lists, a free list, a recursive prune of the
 *                   leaves when the table is found full, a 32-bit code buffer spilled four bytes at a time.
 *   shrink_closed : the form the GPU kernel uses (csrc/zada_shrink.hip) -- parent / suffix per node, a "has a child" bit per node, a hashed
 *                   (prefix, suffix) -> code table with linear probing (the first hit in probe order is the earliest added), the partial clear
 *                   as "every code >= 257 without a child at that moment", the free list as a set read in ascending order, a plain LSB-first bit stream.
 *   shrink_decode : a decoder written from APPNOTE 5.1.
 *
 * Both encoders fill a census (SHRINK_CENSUS values); the two forms give the same bytes exactly when the "should not happen" counts are zero.
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

enum { SPECIAL = 256, FIRST = 257, MINB = 9, MAXB = 13, TLAST = (1 << MAXB) - 1, UNUSED = -1 };
enum { C_CLEARS, C_RISES, C_DUP_ADDS, C_ADD_UNDER_FREED, C_ALLOC_WITH_CHILD, C_UNREACHABLE, C_FULL_NONLITERAL, SHRINK_CENSUS };

typedef struct { uint8_t *out; uint64_t cap, len; } Sink;
static void put_byte(Sink *s, uint8_t b) { if (s->len < s->cap) s->out[s->len] = b; s->len++; }

/* ------------------------------------------------------------------ the stated form */
typedef struct { int child, sibling, suffix; } Rec;
typedef struct {
  Rec t[TLAST + 1];
  int free_list[TLAST + 1], next_free;
  uint8_t clear_list[TLAST + 1];
  uint32_t bit_buffer; int valid_bits, code_size, max_code;
  Sink *s; uint64_t *cs;
} St;

static void st_put_code(St *m, uint32_t code) {
  m->bit_buffer |= m->valid_bits >= 32 ? 0u : code << m->valid_bits;
  m->valid_bits += m->code_size;
  if (m->valid_bits > 32) {
    for (int k = 0; k < 4; k++) put_byte(m->s, (uint8_t)(m->bit_buffer >> (8 * k)));
    m->valid_bits -= 32;
    m->bit_buffer = code >> (m->code_size - m->valid_bits);
  }
}
static void st_prune(St *m, int parent) {
  int cur = m->t[parent].child, sib;
  while (cur != UNUSED && m->t[cur].child == UNUSED) {
    m->t[parent].child = m->t[cur].sibling;
    m->t[cur].sibling = UNUSED;
    m->clear_list[cur] = 1;
    cur = m->t[parent].child;
  }
  if (cur == UNUSED) return;
  st_prune(m, cur);
  sib = m->t[cur].sibling;
  while (sib != UNUSED) {
    if (m->t[sib].child == UNUSED) {
      m->t[cur].sibling = m->t[sib].sibling;
      m->t[sib].sibling = UNUSED;
      m->clear_list[sib] = 1;
    } else {
      cur = sib;
      st_prune(m, cur);
    }
    sib = m->t[cur].sibling;
  }
}
static void st_clear(St *m) {
  /* census: nodes >= 257 that no walk from the 256 roots reaches (the table is full: every node is allocated) */
  static int stack[TLAST + 1];
  static uint8_t seen[TLAST + 1];
  memset(seen, 0, sizeof seen);
  for (int r = 0; r < 256; r++) {
    int sp = 0;
    if (m->t[r].child != UNUSED) stack[sp++] = m->t[r].child;
    while (sp) {
      int c = stack[--sp];
      seen[c] = 1;
      if (m->t[c].sibling != UNUSED) stack[sp++] = m->t[c].sibling;
      if (m->t[c].child != UNUSED) stack[sp++] = m->t[c].child;
    }
  }
  for (int c = FIRST; c <= TLAST; c++) if (!seen[c]) m->cs[C_UNREACHABLE]++;
  memset(m->clear_list, 0, sizeof m->clear_list);
  for (int r = 0; r < 256; r++) st_prune(m, r);
  m->next_free = TLAST + 1;
  for (int c = TLAST; c >= FIRST; c--) if (m->clear_list[c]) m->free_list[--m->next_free] = c;
}
static int st_lookup(St *m, int prefix, int suffix) {
  for (int i = m->t[prefix].child; i != UNUSED; i = m->t[i].sibling) if (m->t[i].suffix == suffix) return i;
  return UNUSED;
}
static void st_add(St *m, int prefix, int suffix) {
  if (m->next_free > TLAST) return;
  int node = m->free_list[m->next_free++];
  if (m->t[node].child != UNUSED) m->cs[C_ALLOC_WITH_CHILD]++;
  m->t[node].child = UNUSED; m->t[node].sibling = UNUSED; m->t[node].suffix = suffix;
  if (m->t[prefix].child == UNUSED) m->t[prefix].child = node;
  else {
    int p = m->t[prefix].child;
    while (m->t[p].sibling != UNUSED) p = m->t[p].sibling;
    m->t[p].sibling = node;
  }
}

uint64_t shrink_stated(const uint8_t *in, uint64_t n, uint8_t *out, uint64_t cap, uint64_t *census) {
  uint64_t dummy[SHRINK_CENSUS];
  Sink s = {out, cap, 0};
  St *m = (St *)malloc(sizeof(St));
  if (!census) census = dummy;
  memset(census, 0, sizeof(uint64_t) * SHRINK_CENSUS);
  m->s = &s; m->cs = census;
  for (int i = 0; i <= TLAST; i++) {
    m->t[i].child = m->t[i].sibling = UNUSED; m->t[i].suffix = i <= 255 ? i : 0;
    m->free_list[i] = i;
  }
  m->next_free = FIRST;
  m->bit_buffer = 0; m->valid_bits = 0; m->code_size = MINB; m->max_code = (1 << MINB) - 1;
  int last = 0;
  for (uint64_t i = 0; i < n; i++) {
    const int suffix = in[i];
    if (i == 0) { last = suffix; continue; }
    if (m->next_free > TLAST) {                       /* the table is full */
      if (last >= 256) census[C_FULL_NONLITERAL]++;
      st_put_code(m, (uint32_t)last); st_put_code(m, SPECIAL); st_put_code(m, 2);
      st_clear(m);
      census[C_CLEARS]++;
      if (st_lookup(m, last, suffix) != UNUSED) census[C_DUP_ADDS]++;
      if (last >= FIRST && m->clear_list[last]) census[C_ADD_UNDER_FREED]++;
      st_add(m, last, suffix);
      last = suffix;
      continue;
    }
    const int at = st_lookup(m, last, suffix);
    if (at != UNUSED) { last = at; continue; }
    st_put_code(m, (uint32_t)last);
    st_add(m, last, suffix);
    last = suffix;
    if (m->code_size < MAXB && m->next_free <= TLAST && m->free_list[m->next_free] > m->max_code) {
      st_put_code(m, SPECIAL); st_put_code(m, 1);
      m->code_size++; m->max_code = (1 << m->code_size) - 1;
      census[C_RISES]++;
    }
  }
  if (n) {
    st_put_code(m, (uint32_t)last);
    while (m->valid_bits > 0) {
      put_byte(&s, (uint8_t)m->bit_buffer);
      m->bit_buffer >>= 8;
      m->valid_bits = m->valid_bits > 8 ? m->valid_bits - 8 : 0;
    }
  }
  free(m);
  return s.len;
}

/* ------------------------------------------------------------------ the closed form */
/* The free list is ascending whenever it is made (at the start, and by every clear) and is read from its front, so it is a set and a cursor:
   is_free [c], the lowest free code from `cursor` on, and a count. */
enum { HSIZE = 12288, HEMPTY = 0xFFFF };
typedef struct {
  uint16_t parent[TLAST + 1], hash[HSIZE];
  uint8_t suf[TLAST + 1], has_child[TLAST + 1], is_free[TLAST + 2];
  int cursor, nfree;
} Cl;
static uint32_t cl_hash(int prefix, int suffix) { return (uint32_t)(((uint64_t)((uint32_t)(prefix * 256 + suffix) * 2654435761u) * HSIZE) >> 32); }
static int cl_next_free(Cl *m) { while (!m->is_free[m->cursor]) m->cursor++; return m->cursor; }     /* (the caller has counted that there is one) */
static int cl_lookup(const Cl *m, int prefix, int suffix) {
  for (uint32_t h = cl_hash(prefix, suffix);; h = h + 1 == HSIZE ? 0 : h + 1) {
    const int v = m->hash[h];
    if (v == HEMPTY) return UNUSED;
    if (m->parent[v] == prefix && m->suf[v] == suffix) return v;
  }
}
static void cl_insert(Cl *m, int node) {
  uint32_t h = cl_hash(m->parent[node], m->suf[node]);
  while (m->hash[h] != HEMPTY) h = h + 1 == HSIZE ? 0 : h + 1;
  m->hash[h] = (uint16_t)node;
}
static void cl_add(Cl *m, int prefix, int suffix) {
  if (m->nfree == 0) return;
  const int node = cl_next_free(m);
  m->is_free[node] = 0; m->nfree--;
  m->parent[node] = (uint16_t)prefix; m->suf[node] = (uint8_t)suffix; m->has_child[node] = 0;
  m->has_child[prefix] = 1;
  cl_insert(m, node);
}

uint64_t shrink_closed(const uint8_t *in, uint64_t n, uint8_t *out, uint64_t cap, uint64_t *census) {
  uint64_t dummy[SHRINK_CENSUS];
  Sink s = {out, cap, 0};
  Cl *m = (Cl *)malloc(sizeof(Cl));
  if (!census) census = dummy;
  memset(census, 0, sizeof(uint64_t) * SHRINK_CENSUS);
  memset(m->hash, 0xFF, sizeof m->hash);
  memset(m->has_child, 0, sizeof m->has_child);
  for (int c = 0; c <= TLAST + 1; c++) m->is_free[c] = c >= FIRST && c <= TLAST;
  m->cursor = FIRST; m->nfree = TLAST + 1 - FIRST;
  uint64_t acc = 0; int nacc = 0;                    /* the bit stream, LSB first */
  int code_size = MINB, max_code = (1 << MINB) - 1, last = 0;
#define PUT(c) do { acc |= (uint64_t)(c) << nacc; nacc += code_size; while (nacc >= 8) { put_byte(&s, (uint8_t)acc); acc >>= 8; nacc -= 8; } } while (0)
  for (uint64_t i = 0; i < n; i++) {
    const int suffix = in[i];
    if (i == 0) { last = suffix; continue; }
    if (m->nfree == 0) {
      if (last >= 256) census[C_FULL_NONLITERAL]++;
      PUT(last); PUT(SPECIAL); PUT(2);
      int cnt = 0;
      for (int c = FIRST; c <= TLAST; c++) { m->is_free[c] = !m->has_child[c]; cnt += m->is_free[c]; }   /* the leaves */
      m->cursor = FIRST; m->nfree = cnt;
      memset(m->hash, 0xFF, sizeof m->hash);
      {
        static uint8_t was[TLAST + 1];
        memcpy(was, m->has_child, sizeof was);
        memset(m->has_child, 0, sizeof m->has_child);
        for (int c = FIRST; c <= TLAST; c++) if (was[c]) { m->has_child[m->parent[c]] = 1; cl_insert(m, c); }
        if (last >= FIRST && !was[last]) census[C_ADD_UNDER_FREED]++;
      }
      census[C_CLEARS]++;
      if (cl_lookup(m, last, suffix) != UNUSED) census[C_DUP_ADDS]++;
      cl_add(m, last, suffix);
      last = suffix;
      continue;
    }
    const int at = cl_lookup(m, last, suffix);
    if (at != UNUSED) { last = at; continue; }
    PUT(last);
    cl_add(m, last, suffix);
    last = suffix;
    if (code_size < MAXB && m->nfree && cl_next_free(m) > max_code) {
      PUT(SPECIAL); PUT(1);
      code_size++; max_code = (1 << code_size) - 1;
      census[C_RISES]++;
    }
  }
  if (n) {
    PUT(last);
    if (nacc) put_byte(&s, (uint8_t)acc);
  }
#undef PUT
  free(m);
  return s.len;
}

/* ------------------------------------------------------------------ the decoder (APPNOTE 5.1) */
/* returns the bytes written, or -1 for a damaged stream; stops at cap bytes or when fewer bits than one code are left */
int64_t shrink_decode(const uint8_t *in, uint64_t n_in, uint8_t *out, uint64_t cap) {
  static int parent[TLAST + 1];
  static uint8_t value[TLAST + 1], stack[TLAST + 2], is_parent[TLAST + 1];
  enum { FREE = -2 };
  for (int c = 0; c <= TLAST; c++) { parent[c] = c < 256 ? UNUSED : FREE; value[c] = (uint8_t)c; }
  uint64_t bitpos = 0, olen = 0;
  const uint64_t nbits = n_in * 8;
  int code_size = MINB, old = UNUSED, finchar = 0;
#define GET(v) do { if (bitpos + code_size > nbits) return (int64_t)olen; uint32_t w_ = 0; for (int k_ = 0; k_ < code_size; k_++, bitpos++) w_ |= (uint32_t)((in[bitpos >> 3] >> (bitpos & 7)) & 1) << k_; (v) = (int)w_; } while (0)
  while (olen < cap) {
    int code;
    GET(code);
    if (code == SPECIAL) {
      int sub;
      GET(sub);
      if (sub == 1) { if (code_size >= MAXB) return -1; code_size++; }
      else if (sub == 2) {                               /* partial clear: every code from 257 on that is nobody's prefix becomes free */
        memset(is_parent, 0, sizeof is_parent);
        for (int c = FIRST; c <= TLAST; c++) if (parent[c] != FREE && parent[c] >= 0) is_parent[parent[c]] = 1;
        for (int c = FIRST; c <= TLAST; c++) if (!is_parent[c]) parent[c] = FREE;
      } else return -1;
      continue;
    }
    if (old == UNUSED) {                                 /* the first code is a byte */
      if (code > 255) return -1;
      out[olen++] = (uint8_t)code; finchar = code; old = code;
      continue;
    }
    int sp = 0, cur = code;
    if (code >= FIRST && parent[code] == FREE) { stack[sp++] = (uint8_t)finchar; cur = old; }   /* the code that is being defined */
    while (cur >= FIRST) {
      if (parent[cur] == FREE || sp > TLAST) return -1;
      stack[sp++] = value[cur];
      cur = parent[cur];
    }
    if (cur < 0 || cur > 255) return -1;
    finchar = cur;
    stack[sp++] = (uint8_t)cur;
    while (sp && olen < cap) out[olen++] = stack[--sp];
    if (sp) return -1;
    int f = FIRST;                                       /* the lowest free code takes (old, first byte of this string) */
    while (f <= TLAST && parent[f] != FREE) f++;
    if (f <= TLAST) { parent[f] = old; value[f] = (uint8_t)finchar; }
    old = code;
  }
#undef GET
  return (int64_t)olen;
}

/* Seeded self-test over `count` small inputs of 0 .. 3 000 bytes: returns how many inputs fail (stated != closed, decoder != input, or a
 * "should not happen" count above zero).  Used by tests/test_legacy_model.py and by the sanitizer program (tests/legacy/legacy_check_main.c). */
static uint32_t lcg(uint32_t *s) { *s = *s * 1664525u + 1013904223u; return *s >> 8; }
int shrink_check_one(const uint8_t *d, uint64_t n, uint64_t *census_sum) {
  const uint64_t cap = n * 5 + 64;
  uint8_t *a = (uint8_t *)malloc(cap), *b = (uint8_t *)malloc(cap), *back = (uint8_t *)malloc(n + 1);
  uint64_t ca[SHRINK_CENSUS], cb[SHRINK_CENSUS];
  const uint64_t la = shrink_stated(d, n, a, cap, ca), lb = shrink_closed(d, n, b, cap, cb);
  int bad = la != lb || la > cap || memcmp(a, b, la) != 0 || memcmp(ca, cb, sizeof ca) != 0;
  bad |= ca[C_ADD_UNDER_FREED] || ca[C_ALLOC_WITH_CHILD] || ca[C_UNREACHABLE] || ca[C_FULL_NONLITERAL];
  if (!bad) bad = shrink_decode(a, la, back, n) != (int64_t)n || memcmp(back, d, n) != 0;
  if (census_sum) for (int k = 0; k < SHRINK_CENSUS; k++) census_sum[k] += ca[k];
  free(a); free(b); free(back);
  return bad;
}
int shrink_selftest(uint32_t seed, int count, uint64_t *census_sum) {
  int bad = 0;
  uint8_t *d = (uint8_t *)malloc(3001);
  for (int t = 0; t < count; t++) {
    uint32_t s = seed + (uint32_t)t * 7919u;
    const uint64_t n = lcg(&s) % 3001;
    const uint32_t alpha = 1 + lcg(&s) % (t % 3 == 0 ? 256 : 6);
    for (uint64_t i = 0; i < n; i++) d[i] = (uint8_t)(lcg(&s) % alpha + (alpha < 100 ? 'a' : 0));
    bad += shrink_check_one(d, n, census_sum);
  }
  free(d);
  return bad;
}
