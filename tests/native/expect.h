// What the host-sanitized programs of this folder share: a failure count,
// EXPECT (report and count, go on), named (the last error names the entry
// point) and finish (the closing line and the exit status).
#pragma once
#include <cstdio>
#include <cstring>

#include "hybridflux.h"

static int g_fail = 0;
#define EXPECT(cond)                                                   \
  do {                                                                 \
    if (!(cond)) {                                                     \
      std::fprintf(stderr, "FAIL %s:%d: %s (%s)\n", __FILE__, __LINE__, #cond, hf_last_error()); \
      ++g_fail;                                                        \
    }                                                                  \
  } while (0)

[[maybe_unused]] static bool named(const char *fn) { return std::strstr(hf_last_error(), fn) != nullptr; }

// "<name>: clean" and 0, or "<name>: N failure(s)" and 1: main's return value
static int finish(const char *name) {
  if (g_fail) {
    std::fprintf(stderr, "%s: %d failure(s)\n", name, g_fail);
    return 1;
  }
  std::printf("%s: clean\n", name);
  return 0;
}
