// stage_check.cpp -- Stage (myriad_amd/csrc/host_stage.h) on a malloc / memcpy backend, as a program of its own for the host sanitizers:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan stage_check.cpp -o stage_check && ./stage_check
// The registration lists are those of myr_eval, myr_solve, myr_solve_x0 and of the restoration working set (myriad_hip.hip), at odd sizes, with every
// optional array present and absent, for host and device callers.  Exit status 0 and "stage_check: ok" when every check holds.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <deque>
#include <vector>

#include "../../myriad_amd/csrc/host_stage.h"

static int g_checks = 0;
#define CHECK(cond)                                                                  \
  do {                                                                               \
    ++g_checks;                                                                      \
    if (!(cond)) { fprintf(stderr, "stage_check: line %d: %s\n", __LINE__, #cond); exit(1); } \
  } while (0)

// the "device": one buffer of exactly the size asked for (an overrun is the sanitizer's to find), and a log of what was copied
struct Mem {
  char* buf = nullptr; size_t have = 0, last_need = 0; int grows = 0, syncs = 0;
  std::vector<const void*> ups, downs;      // device addresses, in the order of the copies
  ~Mem() { free(buf); }
};
struct MemBackend {
  Mem* m;
  int grow(size_t need, void** base) {
    m->last_need = need;
    if (need > m->have) { free(m->buf); m->buf = (char*)malloc(need); m->have = need; ++m->grows; }
    *base = m->buf;
    return 0;
  }
  int upload(void* dev, const void* host, size_t bytes) { memcpy(dev, host, bytes); m->ups.push_back(dev); return 0; }
  int download(void* host, const void* dev, size_t bytes) { memcpy(host, dev, bytes); m->downs.push_back(dev); return 0; }
  int sync() { ++m->syncs; return 0; }
};

enum Kind { IN, OUT, INOUT, SCRATCH, OUT_ALWAYS };
constexpr size_t GUARD = 32;
static unsigned char pat(int id, size_t i, int salt) { return (unsigned char)(id * 37 + i * 11 + salt); }

// one registered array: the caller's side (allocated apart from the device buffer, guard bytes behind it) and the pointer variable Stage fills
struct Rec {
  Kind kind; size_t esz, count; unsigned char* user = nullptr;
  double* vd = nullptr; const double* vcd = nullptr; int32_t* vi = nullptr;
  size_t bytes() const { return esz * count; }
  const void* dev() const { return esz == 4 ? (const void*)vi : (kind == IN ? (const void*)vcd : (const void*)vd); }
};

struct Call {
  Mem* mem; bool host; myriad::Stage<MemBackend> st; std::deque<Rec> recs;
  Call(Mem* m, bool host_) : mem(m), host(host_), st(MemBackend{m}, host_) {}
  ~Call() { for (Rec& r : recs) free(r.user); }
  Rec& make(Kind k, size_t esz, size_t count, bool present) {
    recs.push_back(Rec{k, esz, count});
    Rec& r = recs.back();
    if (present && k != SCRATCH) {
      r.user = (unsigned char*)malloc(r.bytes() + GUARD);
      for (size_t i = 0; i < r.bytes(); ++i) r.user[i] = pat((int)recs.size(), i, 1);
      memset(r.user + r.bytes(), 0xA5, GUARD);
    }
    return r;
  }
  void in(size_t count, bool present = true) { Rec& r = make(IN, 8, count, present); st.in(r.vcd, (const double*)r.user, count); }
  void out(size_t count, bool present = true) { Rec& r = make(OUT, 8, count, present); st.out(r.vd, (double*)r.user, count); }
  void inout(size_t count) { Rec& r = make(INOUT, 8, count, true); st.inout(r.vd, (double*)r.user, count); }
  void scratch(size_t count) { Rec& r = make(SCRATCH, 8, count, false); st.scratch(r.vd, count); }
  void scratch32(size_t count) { Rec& r = make(SCRATCH, 4, count, false); st.scratch(r.vi, count); }
  void always(size_t count, bool present) { Rec& r = make(OUT_ALWAYS, 8, count, present); st.out(r.vd, (double*)r.user, count, true); }
  void always32(size_t count, bool present) { Rec& r = make(OUT_ALWAYS, 4, count, present); st.out(r.vi, (int32_t*)r.user, count, true); }

  bool expect_staged(const Rec& r) const {
    if (!r.count) return false;
    if (r.kind == SCRATCH) return true;
    return host && (r.user || r.kind == OUT_ALWAYS);
  }
  // commit, every check on the layout and the uploads, a pattern over every carve, finish, every check on the downloads
  void run() {
    const int grows0 = mem->grows; const size_t have0 = mem->have;
    mem->ups.clear(); mem->downs.clear(); mem->syncs = 0;
    CHECK(st.commit() == 0);
    CHECK(st.count() == (int)recs.size());
    size_t payload = 0;
    std::vector<std::pair<const char*, size_t>> carves;
    std::vector<const void*> want_ups, want_downs;
    for (size_t i = 0; i < recs.size(); ++i) {
      const Rec& r = recs[i];
      const char* d = (const char*)r.dev();
      CHECK(st.staged((int)i) == expect_staged(r));
      CHECK(st.device((int)i) == (void*)d && st.bytes((int)i) == r.bytes());
      if (!expect_staged(r)) {      // a device caller's own pointer; null for a host caller, an absent array or a zero count
        CHECK(d == ((!host && r.count) ? (const char*)r.user : nullptr));
        continue;
      }
      payload += r.bytes();
      CHECK(((uintptr_t)d & 15) == 0);
      CHECK(d >= mem->buf && d + r.bytes() <= mem->buf + mem->last_need);
      carves.push_back({d, r.bytes()});
      if (r.kind == IN || r.kind == INOUT) { CHECK(memcmp(d, r.user, r.bytes()) == 0); want_ups.push_back(d); }
      if ((r.kind == OUT || r.kind == INOUT || r.kind == OUT_ALWAYS) && r.user) want_downs.push_back(d);
    }
    CHECK(mem->ups == want_ups);      // the registered inputs, in registration order, nothing else
    CHECK(mem->last_need <= payload + 16 * recs.size());
    CHECK(mem->last_need <= mem->have);
    CHECK(mem->grows == grows0 + (mem->last_need > have0 ? 1 : 0));
    if (carves.empty()) CHECK(mem->grows == grows0);
    std::sort(carves.begin(), carves.end());
    for (size_t i = 1; i < carves.size(); ++i) CHECK(carves[i - 1].first + carves[i - 1].second <= carves[i].first);
    // a pattern of its own over every carve's full extent; afterwards every carve still holds its own
    for (size_t i = 0; i < recs.size(); ++i)
      if (expect_staged(recs[i])) { unsigned char* d = (unsigned char*)recs[i].dev(); for (size_t k = 0; k < recs[i].bytes(); ++k) d[k] = pat((int)i + 1, k, 2); }
    for (size_t i = 0; i < recs.size(); ++i)
      if (expect_staged(recs[i])) { const unsigned char* d = (const unsigned char*)recs[i].dev(); for (size_t k = 0; k < recs[i].bytes(); ++k) CHECK(d[k] == pat((int)i + 1, k, 2)); }
    CHECK(st.finish() == 0);
    CHECK(mem->syncs == (host ? 1 : 0));
    if (!host) want_downs.clear();
    CHECK(mem->downs == want_downs);
    for (size_t i = 0; i < recs.size(); ++i) {
      const Rec& r = recs[i];
      if (!r.user) continue;
      const bool down = host && r.kind != IN && expect_staged(r);
      for (size_t k = 0; k < r.bytes(); ++k) CHECK(r.user[k] == (down ? pat((int)i + 1, k, 2) : pat((int)i + 1, k, 1)));      // exactly the registered count ...
      for (size_t k = 0; k < GUARD; ++k) CHECK(r.user[r.bytes() + k] == 0xA5);                                              // ... and not a byte more
    }
  }
};

// CARTPOLE, Hermite-Simpson, 3 intervals: n = 35, m = 24; np = 5 keeps the parameter rows odd too
constexpr size_t n = 35, m = 24, np = 5, ns = 4, nu = 1, ngrad = 7, jblk = 300;
static size_t npar(int pm, size_t B) { return pm == 0 ? 0 : (pm == 1 ? np : B * np); }

static void reg_eval(Call& c, size_t B, int pm, int outs) {
  c.in(B * n); c.in(npar(pm, B), pm != 0);
  c.out(B, outs & 1); c.out(B * ngrad, outs & 2); c.out(B * m, outs & 4); c.out(B * jblk, outs & 8);
}
static void reg_solve_tail(Call& c, size_t B, int pm, int res) {
  c.out(B * m, res & 1); c.in(npar(pm, B), pm != 0);
  c.always(B, res & 2); c.always32(B, res & 4); c.always32(B, res & 8); c.always(3 * B, res & 16);
}
static void reg_solve(Call& c, size_t B, int pm, int res) {
  c.inout(B * n); c.in(B * n); c.in(B * n);
  reg_solve_tail(c, B, pm, res);
}
static void reg_solve_x0(Call& c, size_t B, int pm, int res) {
  c.scratch(B * n); c.scratch(B * n);
  c.out(B * n); c.in(B * ns);
  for (int k = 0; k < 4; ++k) c.in(n);
  reg_solve_tail(c, B, pm, res);
}
static void reg_restore(Call& c, size_t F, bool twin, bool starts) {
  const size_t nt = 7 * (ns + nu + ns), steps = 6, rr = 7;
  c.scratch32(F); c.scratch32(F);
  for (int k = 0; k < 4; ++k) c.scratch(F * n);
  c.scratch(F * np); c.scratch(F * m); c.scratch(F); c.scratch(F * 3); c.scratch32(F); c.scratch32(F);
  if (twin) { for (int k = 0; k < 3; ++k) c.scratch(F * nt); c.scratch(F * (np + 1)); c.scratch(F); c.scratch(64); }
  if (starts) { c.scratch(F * rr * nu); c.scratch(F * ns); c.scratch(F * (steps + 1) * ns); }
}

int main() {
  const size_t Bs[2] = {1, 3};
  for (int host = 0; host < 2; ++host)
    for (size_t B : Bs)
      for (int pm = 0; pm < 3; ++pm) {
        for (int outs = 0; outs < 16; ++outs) { Mem mem; Call c(&mem, host); reg_eval(c, B, pm, outs); c.run(); }
        for (int res = 0; res < 32; ++res) {
          { Mem mem; Call c(&mem, host); reg_solve(c, B, pm, res); c.run(); }
          { Mem mem; Call c(&mem, host); reg_solve_x0(c, B, pm, res); c.run(); }
        }
      }
  for (size_t F : Bs)
    for (int v = 0; v < 4; ++v) { Mem mem; Call c(&mem, false); reg_restore(c, F, v & 1, v & 2); c.run(); CHECK(c.st.count() <= 24); }
  {      // a device caller reserves the scratch items alone
    Mem mem; Call c(&mem, false); reg_solve_x0(c, 3, 2, 31); c.run();
    CHECK(mem.last_need == 2 * ((3 * n * 8 + 15) & ~(size_t)15));
  }
  {      // a null input and a zero count give a null pointer and no room, whatever the kind
    Mem mem; Call c(&mem, true);
    c.in(0, true); c.in(7, false); c.out(0, true); c.out(7, false); c.scratch(0); c.always(0, true); c.always32(0, false);
    c.run();
    CHECK(mem.grows == 0 && mem.buf == nullptr);
    for (const Rec& r : c.recs) CHECK(r.dev() == nullptr);
  }
  {      // the same buffer again: larger counts grow it once, smaller ones not at all
    Mem mem;
    { Call c(&mem, true); reg_solve(c, 1, 1, 31); c.run(); }
    CHECK(mem.grows == 1);
    { Call c(&mem, true); reg_solve(c, 3, 2, 31); c.run(); }
    CHECK(mem.grows == 2);
    { Call c(&mem, true); reg_eval(c, 1, 0, 4); c.run(); }
    { Call c(&mem, false); reg_solve_x0(c, 1, 0, 0); c.run(); }
    CHECK(mem.grows == 2);
  }
  printf("stage_check: ok (%d checks)\n", g_checks);
  return 0;
}
