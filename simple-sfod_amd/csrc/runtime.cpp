// Error plumbing + version of libsfod_hip.so
#include <stdarg.h>
#include <stdio.h>
#include <string>

#include "common.h"

static thread_local char g_err[512] = "";
static thread_local const char* g_last_conv_kernel = nullptr;
static thread_local const char* g_last_conv_kernel_then = nullptr;

void sfod_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

void sfod_note_conv_kernel(const char* name) {
  g_last_conv_kernel = name;
  g_last_conv_kernel_then = nullptr;
}
void sfod_note_conv_kernel_then(const char* name) { g_last_conv_kernel_then = name; }

std::string sfod_kernel_name(const char* fmt, ...) {
  char buf[160];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  return std::string(buf);
}

extern "C" int sfod_version(void) { return 100; }
extern "C" const char* sfod_last_error(void) { return g_err; }

extern "C" int sfod_last_conv_kernel(char* buf, int n) {
  if (buf == nullptr || n <= 0) {
    sfod_set_error("bad argument: last_conv_kernel: null buffer or n <= 0");
    return SFOD_EBADARG;
  }
  const char* name = g_last_conv_kernel ? g_last_conv_kernel : "";
  if (g_last_conv_kernel_then == nullptr) return snprintf(buf, (size_t)n, "%s", name);
  return snprintf(buf, (size_t)n, "%s+%s", name, g_last_conv_kernel_then);
}
