// plan_check — prints the stack rule of csrc/kernel_plan.h for tests/test_kernel_plan_host.py:
// one line "kind need override stack_entries STACK spills supported" per case (override -1: none).
// build: g++ -std=c++17 -I../metal-renderer_amd/csrc plan_check.cpp
#include <cstdio>

#include "kernel_plan.h"

int main() {
  for (uint32_t kind = 0; kind < 3; ++kind)
    for (int ov : {-1, 8, 12, 16, 24, 32, 40})
      for (uint32_t need = 1; need <= 64; ++need) {
        const mrt::StackChoice c = mrt::stack_rule((mrt::KernelKind)kind, need, ov < 0 ? std::nullopt : std::optional<uint32_t>(ov));
        std::printf("%u %u %d %u %d %d %d\n", kind, need, ov, c.stack_entries, c.stack, (int)c.spills, (int)c.supported);
      }
  return 0;
}
