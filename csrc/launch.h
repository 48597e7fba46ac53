// Host-side helpers of the extern "C" kernel launchers: one way to launch a kernel, and the
// dispatch of a runtime flag to a template argument. Everything here is an inline template, so a
// launcher still makes the same HIP calls: at most one hipFuncSetAttribute, one launch, one
// hipGetLastError.
//
//   return by_dim(a->dim, [&](auto D) {
//     return by_flag(a->acts != nullptr, [&](auto ACTS) {
//       return launch_lds(some_kernel<D(), ACTS()>, grid, block, lds, st, *a);
//     });
//   });
//
// Nesting the helpers instantiates the cross product of their values; where the kernels are not a
// full product (stamps excludes acts, the actuator limit excludes stamps) write the choice out.
// Kernel names and template arguments are part of the profiles and tests: keep them stable.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>
#include <utility>

namespace mb {

template <class Kern, class... Args>
inline int launch(Kern kern, dim3 grid, dim3 block, size_t lds, hipStream_t st, Args&&... args) {
  hipLaunchKernelGGL(kern, grid, block, lds, st, std::forward<Args>(args)...);
  return (int)hipGetLastError();
}

// the same, after raising the kernel's dynamic-LDS limit to `lds` (error ignored: the launch reports)
template <class Kern, class... Args>
inline int launch_lds(Kern kern, dim3 grid, dim3 block, size_t lds, hipStream_t st, Args&&... args) {
  (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  return launch(kern, grid, block, lds, st, std::forward<Args>(args)...);
}

// f(std::integral_constant<int, 3>) for dim == 3, <2> for every other value
template <class F>
inline auto by_dim(int dim, F&& f) {
  return dim == 3 ? f(std::integral_constant<int, 3>{}) : f(std::integral_constant<int, 2>{});
}

template <class F>
inline auto by_flag(bool on, F&& f) {
  return on ? f(std::true_type{}) : f(std::false_type{});
}

// the constant-K instantiations: f(<12>) for K == 12 (TOP_K), f(<0>) = runtime K otherwise
template <class F>
inline auto by_k12(int K, F&& f) {
  return K == 12 ? f(std::integral_constant<int, 12>{}) : f(std::integral_constant<int, 0>{});
}

}  // namespace mb
