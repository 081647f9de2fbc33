// kernel_plan.h — which persistent kernel a renderer runs: its kind, the LDS
// traversal-stack variant of that kind, and the grid.  Pure host code (no HIP):
// renderer.cpp fills a KernelPlan from it, kernels.hip turns the same lists
// into template arguments, tools/plan_check.cpp prints the rule for the tests.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <optional>

namespace mrt {

// the values of mrt_stats::kernel (include/mrt.h)
enum class KernelKind : uint32_t {
  Bounce = 0,   // wavefront: one launch per bounce over compacted ray queues
  Path = 1,     // path megakernel: every bounce of a frame batch in one launch
  Stream = 2,   // wave-local streaming wavefront: one launch, per-wave queues
};

inline uint32_t launches_per_batch(KernelKind kind, uint32_t max_path_length) {
  return kind == KernelKind::Bounce ? max_path_length : 1u;
}

// The template STACK values each kind instantiates: |STACK| LDS entries per
// lane; negative: deeper entries spill to global memory (BounceArgs::
// stack_spill).  Written once: run_stack picks from these lists and
// kernels.hip instantiates exactly them.  The per-bounce kernel has no -12 and
// the stream kernel (whole-scene-in-LDS scenes, shallow trees) no spill
// variant at all.
template <int... S> struct StackList {};
constexpr StackList<-8, -12, -16, -32, 8, 12, 16, 24, 32> kPathStacks{};
constexpr StackList<-8, -16, -32, 8, 12, 16, 24, 32> kBounceStacks{};
constexpr StackList<8, 12, 16, 24, 32> kStreamStacks{};

template <KernelKind K> constexpr auto stacks_of() {
  if constexpr (K == KernelKind::Path) return kPathStacks;
  else if constexpr (K == KernelKind::Bounce) return kBounceStacks;
  else return kStreamStacks;
}

// the list's smallest variant of at least `entries` LDS entries that spills or
// not as asked (each sign is listed in ascending size: the first that fits);
// 0: it has none
template <int... S> constexpr int pick_stack(StackList<S...>, uint32_t entries, bool spills) {
  for (int v : {S...})
    if ((v < 0) == spills && (uint32_t)(v < 0 ? -v : v) >= entries) return v;
  return 0;
}

// The template STACK a kind runs for `entries` LDS entries asked for (a
// renderer's stack_entries): the per-bounce kernel runs -16 for "12, spilling".
// 0: the kind has no such variant (a stream kernel that would spill).
constexpr int run_stack(KernelKind kind, uint32_t entries, bool spills) {
  switch (kind) {
    case KernelKind::Path: return pick_stack(kPathStacks, entries, spills);
    case KernelKind::Bounce: return pick_stack(kBounceStacks, entries, spills);
    case KernelKind::Stream: return pick_stack(kStreamStacks, entries, spills);
  }
  return 0;
}

struct StackChoice {
  uint32_t stack_entries;   // LDS entries the renderer asks for (the same for every kind)
  int stack;                // the template STACK `kind` runs for them; 0 with !supported
  bool spills;              // need > stack_entries: the rest of a lane's stack lives in global memory
  bool supported;           // `kind` has a variant for it
};

// The stack rule.  need: the entries a ray of the scene can need, the deeper
// of the main and the occluder tree (DeviceScene::max_stack: shadow rays may
// traverse either); cap_override: MRT_STACK.
// LDS per block bounds the resident blocks per CU, and for global-memory
// traversal occupancy wins: a bound <= 16 is kept whole in LDS, rounded up to
// 8 / 12 / 16; deeper trees keep 8 entries in LDS and spill the rest (C4 with 8
// LDS entries + spill ran 1.5x faster than with a 32-entry LDS stack).  r3,
// with traversal slack: trees deeper than 32 entries (the 1M-triangle scenes,
// 48) keep 12 — C4 +1.9 %; C3 (26) is best at 8 (12: -0.4 %, C3g -0.9 %), and
// 16 entries lose everywhere (C4 -0.4 %, C3g -2.4 %).
inline StackChoice stack_rule(KernelKind kind, uint32_t need, std::optional<uint32_t> cap_override) {
  const uint32_t cap = cap_override ? std::max<uint32_t>(8, *cap_override) : need <= 16 ? 16 : need > 32 ? 12 : 8;
  const uint32_t want = std::min(need, cap);
  StackChoice c{};
  c.stack_entries = want <= 8 ? 8 : want <= 12 ? 12 : want <= 16 ? 16 : want <= 24 ? 24 : 32;
  // no kind has a -24: 24 entries that would spill become 32, which may hold the whole stack after all
  if (need > c.stack_entries && c.stack_entries == 24) c.stack_entries = 32;
  c.spills = need > c.stack_entries;
  c.stack = run_stack(kind, c.stack_entries, c.spills);
  c.supported = c.stack != 0;
  return c;
}

// what a renderer runs (mrt_renderer::plan, filled by renderer.cpp plan_kernel)
struct KernelPlan {
  KernelKind kind = KernelKind::Path;
  uint32_t stack_entries = 32;
  bool spills = false;
  uint32_t grid = 0;   // persistent grid of the kind's kernel for this scene
};

}  // namespace mrt
