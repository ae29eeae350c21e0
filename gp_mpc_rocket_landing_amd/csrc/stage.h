// stage.h -- the layout of a Stage's arena (internal.h): which host buffers a call stages,
// where each lies, and the host copies into and out of the arena.  Nothing of HIP in here, so
// tests/stage_layout_main.cpp runs it on malloc'd arenas under the sanitizers.
//
// A call declares each buffer once, naming the pointer that will receive its device address:
// in() for pure inputs, then inout() for buffers both read and written back, then out().
// Every buffer starts on a multiple of 256 bytes, in the order declared; total is the arena's
// size and [back_lo, total) the range read back.  A null host pointer is an absent buffer: it
// takes no room and no part in the order, and binds nullptr.  A present buffer of count 0
// takes no room and binds the address its successor gets.  Nothing is copied and no pointer
// written before pack() / bind(), so the sources stay live until then.
#pragma once
#include <cstddef>
#include <cstring>

struct StageLayout {
  struct Entry {
    void *bind;       // the caller's device pointer (a T *), written by bind()
    const void *src;  // host source of pack(), or null
    void *dst;        // host destination of fetch(), or null
    size_t bytes, off;
  };
  static constexpr int kMax = 16;               // the largest call (the QP solve) declares 13
  static constexpr size_t kNone = (size_t)-1;   // off of an absent buffer; back_lo without read-back
  Entry e[kMax];
  int n = 0;
  size_t total = 0, back_lo = kNone;
  const char *refused = nullptr;  // why the declarations cannot be laid out: nothing may be bound
  static size_t pad(size_t b) { return (b + 255) & ~(size_t)255; }

  template <class T> void in(const T **p, const T *src, size_t cnt) { add(p, src, nullptr, src != nullptr, sizeof(T) * cnt); }
  template <class T> void in(T **p, const T *src, size_t cnt) { add(p, src, nullptr, src != nullptr, sizeof(T) * cnt); }
  template <class T> void inout(T **p, T *buf, size_t cnt) { add(p, buf, buf, buf != nullptr, sizeof(T) * cnt); }
  template <class T> void out(T **p, T *dst, size_t cnt) { add(p, nullptr, dst, dst != nullptr, sizeof(T) * cnt); }

  void add(void *bind, const void *src, void *dst, bool present, size_t bytes) {
    if (refused) return;
    if (n == kMax) {
      refused = "more buffers than the table holds";
      return;
    }
    if (!present) {
      e[n++] = Entry{bind, nullptr, nullptr, 0, kNone};
      return;
    }
    if (!dst && back_lo != kNone) {
      refused = "a pure input declared after a buffer that is read back";
      return;
    }
    if (dst && back_lo == kNone) back_lo = total;
    e[n++] = Entry{bind, src, dst, bytes, total};
    total += pad(bytes);
  }
  // the sources into the host arena h (total bytes)
  void pack(char *h) const {
    for (int i = 0; i < n; ++i)
      if (e[i].src && e[i].bytes) memcpy(h + e[i].off, e[i].src, e[i].bytes);
  }
  // every declared pointer to its place in the device arena d, or to null
  void bind(char *d) const {
    for (int i = 0; i < n; ++i) {
      void *p = e[i].off == kNone ? nullptr : d + e[i].off;
      memcpy(e[i].bind, &p, sizeof(p));  // (a T * of any T)
    }
  }
  // the host arena's read-back range out to the destinations
  void fetch(const char *h) const {
    for (int i = 0; i < n; ++i)
      if (e[i].dst && e[i].bytes) memcpy(e[i].dst, h + e[i].off, e[i].bytes);
  }
};
