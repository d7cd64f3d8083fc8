// Host-only pieces shared by every translation unit of libflairhip (ffa_common.h includes this file).
#pragma once
#include "../../include/flairhip.h"

void ffa_set_error(const char* fmt, ...);

#define FFA_REQUIRE(cond, ...)                 \
  do {                                         \
    if (!(cond)) {                             \
      ffa_set_error(__VA_ARGS__);              \
      return FFA_ERR_ARG;                      \
    }                                          \
  } while (0)
