// pybind11 module macbf_gnn_amd._host: the CPU-side native runtime (no HIP dependency).
// Arguments are host buffer addresses, passed by keyword and read through Args (csrc/pyargs.h);
// shapes/dtypes are validated in macbf_gnn_amd/ops/host.py.
#include <pybind11/pybind11.h>

#include "../pyargs.h"
#include "scenario_host.h"

// f, run without the GIL
template <typename R, typename... A>
static auto nogil(R (*f)(A...)) {
  return [f](A... a) { py::gil_scoped_release g; return f(a...); };
}

static int sample_scenarios(py::kwargs kw) {
  Args x("sample_scenarios", kw);
  mbh::ScenarioSpec sp{};
  x("B", sp.B); x("N", sp.N); x("dim", sp.dim); x("M", sp.M); x("L", sp.L); x("r", sp.r);
  x("spread", sp.spread); sp.seed = x.u("seed"); x("max_rounds", sp.max_rounds);
  return x.then(nogil(mbh::sample_scenarios), sp, x.ptr<const float>("obs"), x.ptr<float>("S"), x.ptr<float>("G"),
                x.ptr<int>("status"), x.i("threads"));
}

static float min_pair_distance(py::kwargs kw) {
  Args x("min_pair_distance", kw);
  return x.then(nogil(mbh::min_pair_distance), x.ptr<const float>("p"), x.i("n"), x.i("dim"), x.i("stride"),
                x.f("L"), x.f("cutoff"));
}

static int sample_obstacles(py::kwargs kw) {
  Args x("sample_obstacles", kw);
  return x.then(nogil(mbh::sample_obstacles), x.ptr<float>("out"), x.i("B"), x.i("n_obs"), x.i("points"), x.i("dim"),
                x.f("L"), (uint64_t)x.u("seed"), x.ptr<const float>("circle"), x.ptr<const float>("rect"),
                x.ptr<const float>("sphere"));
}

PYBIND11_MODULE(_host, m) {
  m.doc() = "macbf_gnn_amd host runtime (scenario sampler)";
  m.def("sample_scenarios", &sample_scenarios);
  m.def("sample_obstacles", &sample_obstacles);
  m.def("min_pair_distance", &min_pair_distance);
}
