// Stand-in for <glog/logging.h> in the CPU build of the reference: LOG swallows its message, CHECK prints it and
// aborts when the condition is false.
#pragma once
#include <cstdlib>
#include <iostream>
#include <sstream>

namespace refshim {
struct NullLog {
  template <typename T>
  NullLog &operator<<(const T &) { return *this; }
};
struct FatalLog {
  std::ostringstream os;
  template <typename T>
  FatalLog &operator<<(const T &v) {
    os << v;
    return *this;
  }
  ~FatalLog() {
    std::cerr << "CHECK failed: " << os.str() << std::endl;
    std::abort();
  }
};
struct Voidify {
  void operator&(NullLog &) {}
  void operator&(FatalLog &) {}
};
}  // namespace refshim

#define INFO 0
#define WARNING 1
#define ERROR 2
#define FATAL 3
#define LOG(severity) ::refshim::NullLog()
#define CHECK(cond) (cond) ? (void)0 : ::refshim::Voidify() & ::refshim::FatalLog() << #cond << " "
