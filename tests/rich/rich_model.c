/*
 * rich_model.c -- CPU model of the Deflate_R front end (LZ77.Rich: Rich Geldreich's PROG2.C as restated in the
 * reference's lz77.adb, LZ77_by_Rich), the checker of the GPU match finder and parser (csrc/zada_rich.hip).
 *
 * Two functions, written independently of each other:
 *   rich_restate  -- a literal restatement: the ring `dict` of 4 sectors + MAXMATCH bytes, the hash table and the
 *                    16-bit nextlink / lastlink lists with NIL, Load_Dict, Delete_Data, Hash_Data, Find_Match,
 *                    Dict_Search (non-greedy) and Encode_Rich;
 *   rich_closed   -- the closed form the GPU implements: per 8 KiB sector an independent parse over a window of at
 *                    most the three sectors before it, one (L, P) pair per position searched from length 2.
 * `fill` is the value of the ring bytes the reference never wrote (its `dict` is an uninitialised local array; the
 * library's convention is 0).  Tokens are in the oracle's format: a literal is its byte, a match
 * ZO_TOKEN_MATCH | length << 16 | distance.  *capped counts the searches that stopped at MAXCOMPARES candidates.
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define TOKEN_MATCH 0x80000000u
#define GREEDY 0
#define MAXCOMPARES 4096
#define NIL 0xFFFFu
#define THRESHOLD 2
#define MAXMATCH 258
#define DICTSIZE 32768
#define HASHBITS 13
#define HASHSIZE (1 << HASHBITS)
#define SHIFTBITS ((HASHBITS + THRESHOLD) / (THRESHOLD + 1))
#define SECTORLEN 8192
#define HASH_MASK_1 0x8000u
#define HASH_MASK_2 0x7FFFu

/* ------------------------------------------------------------------------------------------------------------ */
/* the restatement                                                                                                */
/* ------------------------------------------------------------------------------------------------------------ */
typedef struct {
  const uint8_t *in;
  uint64_t n, pos;
  uint8_t dict[DICTSIZE + MAXMATCH];
  uint16_t hash[HASHSIZE], nextlink[DICTSIZE + 1], lastlink[DICTSIZE];
  int32_t matchlength, matchpos;
  uint32_t *tok;
  uint64_t ntok, cap, capped;
} Rich;

static void put(Rich *r, uint32_t t) {
  if (r->ntok < r->cap) r->tok[r->ntok] = t;
  r->ntok++;
}

static int32_t Load_Dict(Rich *r, int32_t dictpos) {
  int32_t i = 0;
  while (r->pos < r->n) {
    r->dict[dictpos + i] = r->in[r->pos++];
    i++;
    if (i == SECTORLEN) break;
  }
  if (dictpos == 0)
    for (int32_t j = 0; j < MAXMATCH; j++) r->dict[j + DICTSIZE] = r->dict[j];
  return i;
}

static void Delete_Data(Rich *r, int32_t dictpos) {
  const int32_t k = dictpos + SECTORLEN;
  for (int32_t i = dictpos; i < k; i++) {
    const uint16_t j = r->lastlink[i];
    if (j & HASH_MASK_1) {
      if (j != NIL) r->hash[j & HASH_MASK_2] = NIL;
    } else {
      r->nextlink[j] = NIL;
    }
  }
}

static void Hash_Data(Rich *r, int32_t dictpos, int32_t bytestodo) {
  if (bytestodo <= THRESHOLD) {
    for (int32_t i = dictpos; i < dictpos + bytestodo; i++) r->nextlink[i] = r->lastlink[i] = NIL;
    return;
  }
  for (int32_t i = dictpos + bytestodo - THRESHOLD; i < dictpos + bytestodo; i++) r->nextlink[i] = r->lastlink[i] = NIL;
  uint16_t j = (uint16_t)((uint16_t)(r->dict[dictpos] << SHIFTBITS) ^ r->dict[dictpos + 1]);
  const int32_t k = dictpos + bytestodo - THRESHOLD;
  for (int32_t i = dictpos; i < k; i++) {
    j = (uint16_t)(((uint16_t)(j << SHIFTBITS) & (HASHSIZE - 1)) ^ r->dict[i + THRESHOLD]);
    r->lastlink[i] = j | HASH_MASK_1;
    r->nextlink[i] = r->hash[j];
    if (r->nextlink[i] != NIL) r->lastlink[r->nextlink[i]] = (uint16_t)i;
    r->hash[j] = (uint16_t)i;
  }
}

static void Find_Match(Rich *r, int32_t dictpos, int32_t startlen) {
  int32_t i = dictpos, j;
  r->matchlength = startlen;
  uint8_t match_byte = r->dict[dictpos + r->matchlength];
  for (int compare_count = 1; compare_count <= MAXCOMPARES; compare_count++) {
    i = r->nextlink[i];
    if (i == NIL) return;
    if (r->dict[i + r->matchlength] == match_byte) {
      j = 0;
      for (;;) {
        if (r->dict[dictpos + j] != r->dict[i + j]) break;
        j++;
        if (j == MAXMATCH) break;
      }
      if (j > r->matchlength) {
        r->matchlength = j;
        r->matchpos = i;
        if (r->matchlength == MAXMATCH) return;
        match_byte = r->dict[dictpos + r->matchlength];
      }
    }
  }
  r->capped++;
}

static void Dict_Search(Rich *r, int32_t dictpos, int32_t bytestodo) {
  int32_t i = dictpos, j = bytestodo, matchlen1, matchpos1;
#define WRITE_LITERAL_POS_I do { put(r, r->dict[i]); i++; j--; } while (0)
  while (j != 0) {
    Find_Match(r, i, THRESHOLD);
    if (r->matchlength > THRESHOLD) {
      matchlen1 = r->matchlength;
      matchpos1 = r->matchpos;
      for (;;) {
        Find_Match(r, i + 1, matchlen1);
        if (r->matchlength > matchlen1) {
          matchlen1 = r->matchlength;
          matchpos1 = r->matchpos;
          WRITE_LITERAL_POS_I;
        } else {
          if (matchlen1 > j) {
            matchlen1 = j;
            if (matchlen1 <= THRESHOLD) { WRITE_LITERAL_POS_I; break; }
          }
          put(r, TOKEN_MATCH | ((uint32_t)matchlen1 << 16) | (((uint32_t)i - (uint32_t)matchpos1) & (DICTSIZE - 1)));
          i += matchlen1;
          j -= matchlen1;
          break;
        }
      }
    } else {
      WRITE_LITERAL_POS_I;
    }
  }
#undef WRITE_LITERAL_POS_I
}

uint64_t rich_restate(const uint8_t *in, uint64_t n, int fill, uint32_t *tok, uint64_t cap, uint64_t *capped) {
  Rich *r = (Rich *)malloc(sizeof(Rich));
  if (!r) return ~0ull;
  r->in = in; r->n = n; r->pos = 0;
  memset(r->dict, fill & 0xFF, sizeof r->dict);
  memset(r->hash, 0xFF, sizeof r->hash);
  memset(r->nextlink, 0xFF, sizeof r->nextlink);
  memset(r->lastlink, 0xFF, sizeof r->lastlink);
  r->matchlength = r->matchpos = 0;
  r->tok = tok; r->ntok = 0; r->cap = cap; r->capped = 0;
  int32_t dictpos = 0, actual_read;
  int deleteflag = 0;
  for (;;) {                                                     /* Encode_Rich */
    if (deleteflag) Delete_Data(r, dictpos);
    actual_read = Load_Dict(r, dictpos);
    if (actual_read == 0) break;
    Hash_Data(r, dictpos, actual_read);
    Dict_Search(r, dictpos, actual_read);
    dictpos += SECTORLEN;
    if (dictpos == DICTSIZE) { dictpos = 0; deleteflag = 1; }
  }
  const uint64_t k = r->ntok;
  if (capped) *capped = r->capped;
  free(r);
  return k;
}

/* ------------------------------------------------------------------------------------------------------------ */
/* the closed form                                                                                                */
/* ------------------------------------------------------------------------------------------------------------ */
typedef struct {
  const uint8_t *in;
  uint64_t n, s0, e, wstart;       /* the sector [s0, e) and its window's first position */
  int fill;
  const uint32_t *prev;            /* nearest earlier hashed position with the same hash, or ~0 */
  uint64_t capped;
} Closed;

/* What a comparison of sector [s0, e) sees at stream offset x: the loaded bytes, then the ring's older contents --
 * the byte 32 KiB before, or `fill` where the ring was never written. */
static inline int view(const Closed *c, uint64_t x) {
  if (x < c->e) return c->in[x];
  return x >= DICTSIZE ? c->in[x - DICTSIZE] : c->fill;
}

static inline int sector_hashed(uint64_t n, uint64_t q) {        /* q has a hash link: 3 bytes left in its sector */
  const uint64_t t0 = q / SECTORLEN * SECTORLEN, te = t0 + SECTORLEN < n ? t0 + SECTORLEN : n;
  return te - t0 > THRESHOLD && q + THRESHOLD < te;
}

static inline uint32_t hash3(const uint8_t *b) { return (((uint32_t)b[0] << 10) ^ ((uint32_t)b[1] << 5) ^ b[2]) & (HASHSIZE - 1); }

/* the longest match for position i (first reached among equals), searched from length 2: L <= 2 means none */
static void LP(Closed *c, uint64_t i, int *L, uint64_t *P) {
  *L = 0; *P = 0;
  if (i >= c->e || !sector_hashed(c->n, i)) return;
  int best = THRESHOLD, steps = 0;
  uint64_t q = c->prev[i];
  while (q != 0xFFFFFFFFu && q >= c->wstart) {
    int len = 0;
    while (len < MAXMATCH && view(c, i + len) == view(c, q + len)) len++;
    if (len > best) { best = len; *P = q; if (best == MAXMATCH) break; }
    if (++steps == MAXCOMPARES) { c->capped++; break; }
    q = c->prev[q];
  }
  *L = best;
}

uint64_t rich_closed(const uint8_t *in, uint64_t n, int fill, uint32_t *tok, uint64_t cap, uint64_t *capped) {
  uint32_t *prev = (uint32_t *)malloc((n ? n : 1) * sizeof(uint32_t));
  uint32_t *head = (uint32_t *)malloc(HASHSIZE * sizeof(uint32_t));
  if (!prev || !head) { free(prev); free(head); return ~0ull; }
  memset(head, 0xFF, HASHSIZE * sizeof(uint32_t));
  for (uint64_t q = 0; q < n; q++) {
    prev[q] = 0xFFFFFFFFu;
    if (!sector_hashed(n, q)) continue;
    const uint32_t h = hash3(in + q);
    prev[q] = head[h];
    head[h] = (uint32_t)q;
  }
  Closed c;
  c.in = in; c.n = n; c.fill = fill & 0xFF; c.prev = prev; c.capped = 0;
  uint64_t ntok = 0;
#define PUT(t) do { if (ntok < cap) tok[ntok] = (t); ntok++; } while (0)
  for (uint64_t s0 = 0; s0 < n; s0 += SECTORLEN) {
    c.s0 = s0;
    c.e = s0 + SECTORLEN < n ? s0 + SECTORLEN : n;
    c.wstart = s0 >= 3 * SECTORLEN ? s0 - 3 * SECTORLEN : 0;
    uint64_t i = s0, j = c.e - s0;
    while (j > 0) {
      int m, m1;
      uint64_t p, p1;
      LP(&c, i, &m, &p);
      if (m <= THRESHOLD) { PUT(in[i]); i++; j--; continue; }
      for (;;) {
        LP(&c, i + 1, &m1, &p1);
        if (m1 <= m) break;
        PUT(in[i]); i++; j--;
        m = m1; p = p1;
      }
      if ((uint64_t)m > j) {
        m = (int)j;
        if (m <= THRESHOLD) { PUT(in[i]); i++; j--; continue; }
      }
      PUT(TOKEN_MATCH | ((uint32_t)m << 16) | (uint32_t)(i - p));
      i += (uint64_t)m; j -= (uint64_t)m;
    }
  }
#undef PUT
  if (capped) *capped = c.capped;
  free(prev); free(head);
  return ntok;
}
