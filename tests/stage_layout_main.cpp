// The staging layout (csrc/stage.h) on the CPU: malloc'd "pinned" and "device" arenas of exactly
// the computed total, so a total or an offset that is off by one is a heap-overflow report under
// -fsanitize=address.  tests/test_stage_layout.py builds and runs this; exit status 0 is a pass.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../gp_mpc_rocket_landing_amd/csrc/stage.h"

#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      return 1;                                                       \
    }                                                                 \
  } while (0)

// Stage::commit without HIP: refuse, or get both arenas at the total, pack, "upload", bind
static bool commit(const StageLayout &l, char *&h, char *&d) {
  if (l.refused) return false;
  h = (char *)malloc(l.total);
  d = (char *)malloc(l.total);
  memset(h, 0xAA, l.total);
  memset(d, 0x55, l.total);
  l.pack(h);
  memcpy(d, h, l.total);
  l.bind(d);
  return true;
}

// Stage::download without HIP: the read-back range down, then out to the callers' buffers
static void download(const StageLayout &l, char *h, const char *d) {
  if (l.back_lo != StageLayout::kNone) memcpy(h + l.back_lo, d + l.back_lo, l.total - l.back_lo);
  l.fetch(h);
}

static int test_layout_and_round_trip() {
  // byte sizes 8, 248, 0, 256, (absent), 264, 4104, (absent), 8
  double a[1], c[32], e[513], zero_len[1] = {-1.0};
  int b[62], io[66], f[2];
  a[0] = 3.25;
  for (int i = 0; i < 62; ++i) b[i] = 1000 + i;
  for (int i = 0; i < 32; ++i) c[i] = 0.5 * i;
  for (int i = 0; i < 66; ++i) io[i] = 7 * i;
  for (int i = 0; i < 513; ++i) e[i] = -1.0;
  f[0] = f[1] = -1;
  double a0[1], c0[32];
  int b0[62];
  memcpy(a0, a, sizeof a); memcpy(b0, b, sizeof b); memcpy(c0, c, sizeof c);

  char sentinel;
  const double *da = (const double *)&sentinel, *dz = (const double *)&sentinel, *dabs_in = (const double *)&sentinel;
  const int *db = (const int *)&sentinel;
  double *dc = (double *)&sentinel, *de = (double *)&sentinel, *dabs_out = (double *)&sentinel;
  int *dio = (int *)&sentinel, *df = (int *)&sentinel;

  StageLayout l;
  l.in(&da, a, 1);                              // 8 bytes at 0
  l.in(&db, b, 62);                             // 248 bytes at 256
  l.in(&dz, zero_len, 0);                       // present, 0 bytes: at 512, no room
  l.in(&dc, c, 32);                             // 256 bytes at 512 (a non-const device pointer)
  l.in(&dabs_in, (const double *)nullptr, 99);  // absent
  l.inout(&dio, io, 66);                        // 264 bytes at 768: the read-back range starts here
  l.out(&de, e, 513);                           // 4104 bytes at 1280
  l.out(&dabs_out, (double *)nullptr, 99);      // absent
  l.out(&df, f, 2);                             // 8 bytes at 5632
  CHECK(!l.refused);
  CHECK(l.total == 5888);
  CHECK(l.back_lo == 768);
  // declaring writes nothing
  CHECK((const char *)da == &sentinel && (char *)df == &sentinel && (const char *)dabs_in == &sentinel);

  char *h = nullptr, *d = nullptr;
  CHECK(commit(l, h, d));
  CHECK((const char *)da == d + 0);
  CHECK((const char *)db == d + 256);
  CHECK((const char *)dz == d + 512);
  CHECK((char *)dc == d + 512);
  CHECK(dabs_in == nullptr);
  CHECK((char *)dio == d + 768);
  CHECK((char *)de == d + 1280);
  CHECK(dabs_out == nullptr);
  CHECK((char *)df == d + 5632);

  // declared order kept, no two ranges overlap, all inside the arena
  const char *lo[] = {(const char *)da, (const char *)db, (const char *)dz, (const char *)dc,
                      (const char *)dio, (const char *)de, (const char *)df};
  const size_t len[] = {8, 248, 0, 256, 264, 4104, 8};
  for (int i = 0; i < 7; ++i) {
    CHECK(((size_t)(lo[i] - d) & 255) == 0);
    CHECK(lo[i] + len[i] <= (i + 1 < 7 ? lo[i + 1] : d + l.total));
  }

  // the "kernel": reads every input, scribbles over the device copies of the pure inputs, changes
  // the inout, writes the outputs to their last element
  CHECK(da[0] == 3.25);
  for (int i = 0; i < 62; ++i) CHECK(db[i] == 1000 + i);
  for (int i = 0; i < 32; ++i) CHECK(dc[i] == 0.5 * i);
  for (int i = 0; i < 66; ++i) CHECK(dio[i] == 7 * i);
  for (int i = 0; i < 32; ++i) dc[i] = 1e9;
  *(double *)d = 1e9;
  for (int i = 0; i < 66; ++i) dio[i] += 1;
  for (int i = 0; i < 513; ++i) de[i] = 2.0 * i;
  df[0] = 11;
  df[1] = 12;

  download(l, h, d);
  for (int i = 0; i < 66; ++i) CHECK(io[i] == 7 * i + 1);
  for (int i = 0; i < 513; ++i) CHECK(e[i] == 2.0 * i);
  CHECK(f[0] == 11 && f[1] == 12);
  // a pure input's caller buffer is untouched
  CHECK(!memcmp(a, a0, sizeof a) && !memcmp(b, b0, sizeof b) && !memcmp(c, c0, sizeof c));
  CHECK(zero_len[0] == -1.0);
  free(h);
  free(d);
  return 0;
}

// only inputs: nothing is read back
static int test_no_read_back() {
  int v[3] = {1, 2, 3};
  const int *dv = nullptr;
  StageLayout l;
  l.in(&dv, v, 3);
  CHECK(!l.refused && l.total == 256 && l.back_lo == StageLayout::kNone);
  char *h = nullptr, *d = nullptr;
  CHECK(commit(l, h, d));
  CHECK(dv[2] == 3);
  download(l, h, d);
  CHECK(v[0] == 1 && v[1] == 2 && v[2] == 3);
  free(h);
  free(d);
  return 0;
}

static int test_refusals() {
  char sentinel;
  double buf[4] = {0, 0, 0, 0};
  char *h = nullptr, *d = nullptr;
  {  // a full table: kMax declarations pass, one more is refused
    double *p[StageLayout::kMax + 1];
    StageLayout l;
    for (int i = 0; i <= StageLayout::kMax; ++i) {
      p[i] = (double *)&sentinel;
      CHECK(!l.refused);
      l.out(&p[i], buf, 4);
    }
    CHECK(l.refused);
    CHECK(!commit(l, h, d) && !h && !d);
    for (int i = 0; i <= StageLayout::kMax; ++i) CHECK((char *)p[i] == &sentinel);
  }
  {  // an absent buffer fills a slot too
    double *p[StageLayout::kMax + 1];
    StageLayout l;
    for (int i = 0; i <= StageLayout::kMax; ++i) {
      p[i] = (double *)&sentinel;
      l.out(&p[i], (double *)nullptr, 4);
    }
    CHECK(l.refused && !commit(l, h, d));
    for (int i = 0; i <= StageLayout::kMax; ++i) CHECK((char *)p[i] == &sentinel);
  }
  {  // a pure input after an output
    double *po = (double *)&sentinel;
    const double *pi = (const double *)&sentinel;
    StageLayout l;
    l.out(&po, buf, 4);
    l.in(&pi, buf, 4);
    CHECK(l.refused && !commit(l, h, d));
    CHECK((char *)po == &sentinel && (const char *)pi == &sentinel);
  }
  {  // ... or after an inout; later declarations do not lift the refusal
    double *po = (double *)&sentinel, *po2 = (double *)&sentinel;
    const double *pi = (const double *)&sentinel;
    StageLayout l;
    l.inout(&po, buf, 4);
    l.in(&pi, buf, 4);
    l.out(&po2, buf, 4);
    CHECK(l.refused && !commit(l, h, d));
    CHECK((char *)po == &sentinel && (const char *)pi == &sentinel && (char *)po2 == &sentinel);
  }
  {  // an absent input is no part of the order
    double *po = nullptr;
    const double *pi = (const double *)&sentinel;
    StageLayout l;
    l.out(&po, buf, 4);
    l.in(&pi, (const double *)nullptr, 4);
    CHECK(!l.refused && l.total == 256);
    CHECK(commit(l, h, d));
    CHECK((char *)po == d && pi == nullptr);
    free(h);
    free(d);
  }
  return 0;
}

int main() {
  if (test_layout_and_round_trip() || test_no_read_back() || test_refusals()) return 1;
  puts("stage layout ok");
  return 0;
}
