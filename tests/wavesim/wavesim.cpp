// wavesim runtime state — TEST INFRASTRUCTURE ONLY (see wavesim.h).
#include "wavesim.h"
namespace wavesim {
thread_local BlockCtx* g_block = nullptr;
thread_local int g_lane = 0;
thread_local int g_wave = 0;
}  // namespace wavesim
thread_local dim3 threadIdx;
thread_local dim3 blockIdx;
thread_local dim3 blockDim;
thread_local dim3 gridDim;

// ---- launch log: what the host launchers selected (tests/simlib.py reads it through the C functions below) ----
#include <cctype>
#include <cxxabi.h>
#include <map>
#include <mutex>
#include <string>
namespace {
struct LaunchRecord {
  const std::string* name;
  unsigned dims[4];          // grid x, y, z, block x
};
std::mutex g_log_mutex;
std::map<const std::type_info*, std::string> g_names;      // demangled once per instantiation
std::vector<LaunchRecord> g_log;
bool g_dry_run = false;

bool ident_char(char c) { return isalnum((unsigned char)c) || c == '_'; }
// "wavesim::KernelTag<&(void ns::kernel<args>(params))>" -> "ns::kernel<args>(params)"
std::string kernel_name(const char* mangled) {
  std::string m = mangled;
  int status = 0;
  char* d = abi::__cxa_demangle(m.c_str(), nullptr, nullptr, &status);
  bool bf16_as_half = false;
  if (!d) {      // a demangler older than __bf16's mangling (DF16b): demangle it as IEEE half (Dh, a builtin like it, so substitutions keep their numbers)
    for (size_t p; (p = m.find("DF16b")) != std::string::npos;) m.replace(p, 5, "Dh");
    d = abi::__cxa_demangle(m.c_str(), nullptr, nullptr, &status);
    bf16_as_half = true;
  }
  if (!d) return mangled;
  std::string s = d;
  free(d);
  if (bf16_as_half)
    for (size_t p = 0; (p = s.find("half", p)) != std::string::npos; p += 4)
      if ((p == 0 || !ident_char(s[p - 1])) && (p + 4 == s.size() || !ident_char(s[p + 4]))) s.replace(p, 4, "__bf16"), p += 2;
  const std::string pre = "wavesim::KernelTag<&";
  if (s.compare(0, pre.size(), pre) == 0 && s.back() == '>') s = s.substr(pre.size(), s.size() - pre.size() - 1);
  if (s.size() > 2 && s.front() == '(' && s.back() == ')') s = s.substr(1, s.size() - 2);
  if (s.compare(0, 5, "void ") == 0) s.erase(0, 5);
  return s;
}
}  // namespace
bool wavesim::record_launch(const std::type_info& tag, dim3 grid, dim3 block) {
  std::lock_guard<std::mutex> lock(g_log_mutex);
  auto it = g_names.find(&tag);
  if (it == g_names.end()) {
    it = g_names.emplace(&tag, kernel_name(tag.name())).first;
  }
  g_log.push_back(LaunchRecord{&it->second, {grid.x, grid.y, grid.z, block.x}});
  return g_dry_run;
}
extern "C" void wavesim_log_clear(void) {
  std::lock_guard<std::mutex> lock(g_log_mutex);
  g_log.clear();
}
extern "C" int wavesim_log_size(void) {
  std::lock_guard<std::mutex> lock(g_log_mutex);
  return (int)g_log.size();
}
// record i: returns the kernel's name (valid for the life of the process) and fills dims[4] = grid x, y, z, block x; null past the end
extern "C" const char* wavesim_log_get(int i, unsigned* dims) {
  std::lock_guard<std::mutex> lock(g_log_mutex);
  if (i < 0 || i >= (int)g_log.size()) return nullptr;
  for (int k = 0; k < 4; ++k) dims[k] = g_log[i].dims[k];
  return g_log[i].name->c_str();
}
// dry run: launches are recorded and return without executing the kernel body
extern "C" void wavesim_set_dry_run(int on) {
  std::lock_guard<std::mutex> lock(g_log_mutex);
  g_dry_run = on != 0;
}
