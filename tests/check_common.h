// check_common.h -- the harness the stand-alone product check programs (tests/*_check.cpp) share: the check counter, exact-size
// heap arrays, the refusal table's macros, and the hex-float rows the case files and the Python tests exchange.  Each
// program keeps its own cases and its own main, which prints "ok <checks>" at the end.  No project header: a program that
// takes REFUSED or ACCEPTED includes the one that has the TRX_* codes.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <limits>
#include <memory>
#include <string>

inline int g_checks = 0, g_bad = 0;
#define CHECK(cond) do { g_checks++; if (!(cond)) { g_bad++; std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); } } while (0)

// an exact-size heap array (n = 0: a zero-length allocation, not to be read at all): a read past an extent is a sanitizer report
template <class T>
struct Heap {
  std::unique_ptr<T[]> p; size_t n;
  explicit Heap(size_t n_, T fill = T()) : p(new T[n_]), n(n_) { for (size_t i = 0; i < n; i++) p[i] = fill; }
  Heap(std::initializer_list<T> v) : p(new T[v.size()]), n(v.size()) { size_t i = 0; for (const T &x : v) p[i++] = x; }
  T *get() const { return p.get(); }
  T &operator[](size_t i) const { return p[i]; }
};

// a call that leaves its refusal's text in a std::string `msg`: the code and the literal text, or no refusal and no text
inline void refused(int rc, const std::string &msg, int want_rc, const char *want, int line)
{
  g_checks++;
  if (rc == want_rc && msg == want) return;
  g_bad++;
  std::printf("FAILED line %d: got (%d, \"%s\"), want (%d, \"%s\")\n", line, rc, msg.c_str(), want_rc, want);
}
#define REFUSED(call, want_rc, want) do { std::string msg; const int rc_ = (call); refused(rc_, msg, want_rc, want, __LINE__); } while (0)
#define ACCEPTED(call) do { std::string msg = "untouched"; const int rc_ = (call); refused(rc_, msg, TRX_OK, "untouched", __LINE__); } while (0)

constexpr double kNaN = std::numeric_limits<double>::quiet_NaN(), kInf = std::numeric_limits<double>::infinity();

// n doubles of a case file, as words strtod reads (hex floats: exact)
inline std::unique_ptr<double[]> read_doubles(FILE *f, size_t n)
{
  std::unique_ptr<double[]> a(new double[n]);          // exact size: the sanitizer guards both ends
  char word[64];
  for (size_t k = 0; k < n; k++) {
    if (std::fscanf(f, "%63s", word) != 1) { std::fprintf(stderr, "check program: the case file ends early\n"); std::exit(2); }
    a[k] = std::strtod(word, nullptr);
  }
  return a;
}

// a named row of doubles as %a, for the Python test to compare bit for bit
inline void print_doubles(const char *name, const Heap<double> &a)
{
  std::printf("%s", name);
  for (size_t k = 0; k < a.n; k++) std::printf(" %a", a[k]);
  std::printf("\n");
}
