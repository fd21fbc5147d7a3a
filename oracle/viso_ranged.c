/* oracle/viso_ranged.c -- TEST INFRASTRUCTURE ONLY.
 *
 * Plain-C statement of tests/multistage_oracle.py's ranged_matching (Matcher::matching with use_prior = true,
 * DESIGN.md section 6, f-3), for feature sets too large for the per-query Python loop.  It is the project's own
 * code and restates the numpy form line by line: float32 windows query + range, bins of interest from the float
 * window, candidates visited u-bin outer, v-bin inner, list order, first strict minimum, min_ind = 0 when nothing is
 * accepted.  tests/test_multistage_scale.py ties it to the numpy form byte for byte on small scenes. */
#include "viso_oracle.h"
#include <math.h>
#include <stdlib.h>
#include <string.h>

typedef struct {
  const int32_t *m;
  int32_t n;
  int32_t *start; /* [4 * ubn * vbn + 1] */
  int32_t *list;  /* [n] ascending indices per bin (c * vbn + v_bin) * ubn + u_bin */
} rset;

static int32_t bin_of(float x, float bs, int32_t n) {
  float f = floorf(x / bs);
  if (f < 0.0f) f = 0.0f;
  if (f > (float)(n - 1)) f = (float)(n - 1);
  return (int32_t)f;
}

static int build_index(rset *s, float bs, int32_t ubn, int32_t vbn) {
  const int32_t nb = 4 * ubn * vbn;
  s->start = (int32_t *)calloc((size_t)nb + 2, sizeof(int32_t));
  s->list = (int32_t *)malloc(sizeof(int32_t) * (size_t)(s->n > 0 ? s->n : 1));
  int32_t *key = (int32_t *)malloc(sizeof(int32_t) * (size_t)(s->n > 0 ? s->n : 1));
  if (!s->start || !s->list || !key) { free(key); return -1; }
  for (int32_t i = 0; i < s->n; i++) {
    const int32_t *f = s->m + 12 * (size_t)i;
    if (f[3] < 0 || f[3] > 3 || f[0] < 0 || f[1] < 0) { free(key); return -2; }
    key[i] = (f[3] * vbn + bin_of((float)f[1], bs, vbn)) * ubn + bin_of((float)f[0], bs, ubn);
    s->start[key[i] + 2]++;
  }
  for (int32_t b = 0; b < nb; b++) s->start[b + 2] += s->start[b + 1];
  for (int32_t i = 0; i < s->n; i++) s->list[s->start[key[i] + 1]++] = i; /* start[b + 1] ends as the end of bin b */
  free(key);
  return 0;
}

/* findMatch with use_prior = true: -> min_ind; *hit = 1 when a candidate was accepted */
static int32_t find_ranged(const vo_params *p, const rset *q, int32_t i1, const rset *c, int32_t ubn, int32_t vbn, const float *rng,
                           int flow, uint8_t *hit) {
  const float bs = (float)p->match_binsize;
  const int32_t *f1 = q->m + 12 * (size_t)i1;
  const int32_t u1 = f1[0], v1 = f1[1], cls = f1[3];
  const uint8_t *d1 = (const uint8_t *)(f1 + 4);
  float u_min = (float)u1 + rng[0], u_max = (float)u1 + rng[1];
  float v_min = (float)v1 + rng[2], v_max = (float)v1 + rng[3];
  if (!flow) { v_min = (float)(v1 - p->match_disp_tolerance); v_max = (float)(v1 + p->match_disp_tolerance); }
  const int32_t ub0 = bin_of(u_min, bs, ubn), ub1 = bin_of(u_max, bs, ubn);
  const int32_t vb0 = bin_of(v_min, bs, vbn), vb1 = bin_of(v_max, bs, vbn);
  int32_t min_ind = 0, min_cost = 10000000;
  *hit = 0;
  for (int32_t ub = ub0; ub <= ub1; ub++)
    for (int32_t vb = vb0; vb <= vb1; vb++) {
      const int32_t b = (cls * vbn + vb) * ubn + ub;
      for (int32_t k = c->start[b]; k < c->start[b + 1]; k++) {
        const int32_t i2 = c->list[k];
        const int32_t *f2 = c->m + 12 * (size_t)i2;
        const float u2 = (float)f2[0], v2 = (float)f2[1];
        if (!(u2 >= u_min && u2 <= u_max && v2 >= v_min && v2 <= v_max)) continue;
        const uint8_t *d2 = (const uint8_t *)(f2 + 4);
        int32_t cost = 0;
        for (int j = 0; j < 32; j++) cost += abs((int)d1[j] - (int)d2[j]);
        *hit = 1;
        if (cost < min_cost) { min_cost = cost; min_ind = i2; }
      }
    }
  return min_ind;
}

/* stages of a method's circle: query role, candidate role, flow (roles 0 = 1p, 1 = 2p, 2 = 1c, 3 = 2c) */
static const int8_t STAGES[3][4][3] = {
    {{2, 0, 1}, {0, 2, 1}, {-1, 0, 0}, {-1, 0, 0}},
    {{2, 3, 0}, {3, 2, 0}, {-1, 0, 0}, {-1, 0, 0}},
    {{0, 1, 0}, {1, 3, 1}, {3, 2, 0}, {2, 0, 1}},
};

static void put(float *o, const rset *s, int32_t i) {
  int32_t ii = i;
  if (i < 0) { o[0] = -1.0f; o[1] = -1.0f; }
  else { o[0] = (float)s->m[12 * (size_t)i]; o[1] = (float)s->m[12 * (size_t)i + 1]; }
  memcpy(o + 2, &ii, 4);
}

/* ranges: [ubn * vbn][4][4] float.  out: the first `cap` records, *n_out the true count.
 * Optional per-driver outputs (NULL: none): stage_idx[ndrive][4] the answer of every stage (-1: no such stage),
 * stage_hit[ndrive][4] 1 where the stage accepted a candidate, state[ndrive] 0 circle open, 1 emitted,
 * 2 closed and dropped by the first-writer pixel mask (flow), 3 closed and dropped by the u-order test. */
int32_t vo_ranged_matching(const vo_params *p, const int32_t dims[3], int32_t method, const int32_t *m1p, int32_t n1p,
                           const int32_t *m2p, int32_t n2p, const int32_t *m1c, int32_t n1c, const int32_t *m2c, int32_t n2c,
                           const float *ranges, vo_p_match *out, int32_t cap, int32_t *n_out, int32_t *stage_idx,
                           uint8_t *stage_hit, uint8_t *state) {
  if (!p || !dims || !ranges || !n_out || method < 0 || method > 2 || p->match_binsize <= 0) return -1;
  *n_out = 0;
  const float bs = (float)p->match_binsize;
  const int32_t ubn = (int32_t)ceilf((float)dims[0] / bs), vbn = (int32_t)ceilf((float)dims[1] / bs);
  rset s[4] = {{m1p, n1p, 0, 0}, {m2p, n2p, 0, 0}, {m1c, n1c, 0, 0}, {m2c, n2c, 0, 0}};
  static const int8_t NEED[3][4] = {{1, 0, 1, 0}, {0, 0, 1, 1}, {1, 1, 1, 1}};
  for (int r = 0; r < 4; r++) if (NEED[method][r] && s[r].n <= 0) return 0;
  int32_t rc = 0;
  uint8_t *seen = NULL;
  for (int r = 0; r < 4 && !rc; r++) {
    if (!NEED[method][r]) s[r].n = 0;
    rc = build_index(&s[r], bs, ubn, vbn);
  }
  if (!rc && method == 0) { seen = (uint8_t *)calloc((size_t)dims[0] * dims[1], 1); if (!seen) rc = -1; }
  const rset *drive = method == 2 ? &s[0] : &s[2];
  int32_t n = 0;
  for (int32_t i = 0; i < drive->n && !rc; i++) {
    const int32_t u = drive->m[12 * (size_t)i], v = drive->m[12 * (size_t)i + 1];
    if (u >= dims[0] || v >= dims[1]) { rc = -2; break; }
    const int32_t sb = bin_of((float)v, bs, vbn) * ubn + bin_of((float)u, bs, ubn);
    int32_t idx[5] = {i, -1, -1, -1, -1};
    uint8_t hit[4] = {0, 0, 0, 0};
    int nst = 0;
    for (int st = 0; st < 4 && STAGES[method][st][0] >= 0; st++, nst++)
      idx[st + 1] = find_ranged(p, &s[STAGES[method][st][0]], idx[st], &s[STAGES[method][st][1]], ubn, vbn,
                                ranges + ((size_t)sb * 4 + st) * 4, STAGES[method][st][2], &hit[st]);
    if (stage_idx) for (int st = 0; st < 4; st++) stage_idx[4 * (size_t)i + st] = idx[st + 1];
    if (stage_hit) for (int st = 0; st < 4; st++) stage_hit[4 * (size_t)i + st] = hit[st];
    uint8_t stt = 0;
    int32_t rec[4] = {-1, -1, -1, -1};
    if (idx[nst] == i) {
      if (method == 0) {
        if (seen[(size_t)v * dims[0] + u]) stt = 2;
        else { seen[(size_t)v * dims[0] + u] = 1; stt = 1; rec[0] = idx[1]; rec[2] = i; }
      } else if (method == 1) {
        if (u >= s[3].m[12 * (size_t)idx[1]]) { stt = 1; rec[2] = i; rec[3] = idx[1]; } else stt = 3;
      } else {
        const int32_t i2p = idx[1], i2c = idx[2], i1c = idx[3];
        if (u >= s[1].m[12 * (size_t)i2p] && s[2].m[12 * (size_t)i1c] >= s[3].m[12 * (size_t)i2c]) {
          stt = 1; rec[0] = i; rec[1] = i2p; rec[2] = i1c; rec[3] = i2c;
        } else stt = 3;
      }
    }
    if (state) state[i] = stt;
    if (stt == 1) {
      if (n < cap && out) { float *o = (float *)(out + n); for (int r = 0; r < 4; r++) put(o + 3 * r, &s[r], rec[r]); }
      n++;
    }
  }
  for (int r = 0; r < 4; r++) { free(s[r].start); free(s[r].list); }
  free(seen);
  if (rc) return rc;
  *n_out = n;
  return 0;
}
