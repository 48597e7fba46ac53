// Named arguments of the pybind11 layers (_C and _host): one reader for every entry point.
//
// A bound function takes **kwargs, a driver its config dict; both hand the dict to an Args and read
// each value by name -- for a kernel argument struct, the name of the field in csrc/args.h. Args
// takes every value out of its copy of the dict as it reads it, so each key is read once and done()
// sees exactly the keys nothing asked for. A missing key, a key left over and a value of the wrong
// Python type raise TypeError with the entry point and the key, before any HIP call. GIL held.
// Host-only: pybind11 and no HIP header, so csrc/host uses it too.
#pragma once
#include <pybind11/pybind11.h>

#include <cstdint>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <unordered_map>

namespace py = pybind11;
using u64 = unsigned long long;

template <typename T>
inline T* P(u64 p) { return reinterpret_cast<T*>(static_cast<uintptr_t>(p)); }

inline void chk(int rc, const char* what) {
  if (rc != 0) throw std::runtime_error(std::string(what) + " launch failed: " + std::to_string(rc));
}
// a HIP status (hipGetErrorString is looked up where this is used: no HIP header here)
template <typename E, std::enable_if_t<std::is_enum<E>::value, int> = 0>
inline void chk(E e, const char* what) {
  if (e != E{}) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}

// the build of a kernel for precision code 0 (bf16), 1 (fp16), 2 (fp32: the 3-term split)
template <typename F>
inline F by_prec(int prec, F f, F f_f16, F f_x3) {
  if (prec < 0 || prec > 2) throw py::value_error("precision code " + std::to_string(prec) + " outside 0..2");
  return prec == 2 ? f_x3 : prec == 1 ? f_f16 : f;
}

class Args {
 public:
  // reads from a copy of d, which it empties: the caller's dict (or **kwargs) is never touched
  Args(const char* fn, const py::dict& d) : fn_(fn), d_(py::reinterpret_steal<py::dict>(PyDict_Copy(d.ptr()))) {}

  int i(const char* k) { return get<int>(k, "int"); }
  long l(const char* k) { return get<long>(k, "int"); }
  float f(const char* k) { return get<float>(k, "float"); }
  u64 u(const char* k) { return get<u64>(k, "a non-negative int"); }
  template <typename T>
  T* ptr(const char* k) { return P<T>(u(k)); }

  // x("name", a.name) reads a struct field by the field's own type; opt: only if the key is there
  void operator()(const char* k, int& v) { v = i(k); }
  void operator()(const char* k, long& v) { v = l(k); }
  void operator()(const char* k, float& v) { v = f(k); }
  void operator()(const char* k, unsigned& v) { v = get<unsigned>(k, "a non-negative int"); }
  void operator()(const char* k, u64& v) { v = u(k); }
  template <typename T>
  void operator()(const char* k, T*& v) { v = ptr<T>(k); }
  template <typename T>
  void opt(const char* k, T& v) {
    if (PyDict_GetItemWithError(d_.ptr(), key(k))) (*this)(k, v);
    else if (PyErr_Occurred()) throw py::error_already_set();
  }

  // a dict-valued argument, read whole by `fill` (every key of it must be asked for); fn: the name its
  // errors carry. With `none`, None is allowed: *none says so and the result is A{}
  template <typename A>
  A sub(const char* k, const char* fn, A (*fill)(Args&), bool* none = nullptr) {
    py::object v = take(k);
    if (none && (*none = v.is_none())) return A{};
    if (!py::isinstance<py::dict>(v)) wrong_type(k, "a dict", v);
    Args x(fn, py::reinterpret_borrow<py::dict>(v));
    const A a = fill(x);
    x.done();
    return a;
  }

  // loss constants (mb::LossConsts): 7 floats (+ optional device loss-scale pointer)
  template <typename LC>
  LC loss_consts(const char* k) {
    py::object v = take(k);
    if (!py::isinstance<py::tuple>(v) || (py::len(v) != 7 && py::len(v) != 8)) wrong_type(k, "a tuple of 7 or 8", v);
    const py::tuple t = py::reinterpret_borrow<py::tuple>(v);
    try {
      float c[7];
      for (int j = 0; j < 7; ++j) c[j] = t[j].cast<float>();
      return LC{c[0], c[1], c[2], c[3], c[4], c[5], c[6], t.size() > 7 ? P<const float>(t[7].cast<u64>()) : nullptr};
    } catch (const py::cast_error&) {
      wrong_type(k, "7 floats (+ a pointer)", v);
    }
  }

  // after the last read: every key must have been asked for
  void done() {
    if (PyDict_Size(d_.ptr()) == 0) return;
    std::string names;
    for (auto kv : d_) names += (names.empty() ? "'" : ", '") + std::string(py::str(kv.first)) + "'";
    fail("unexpected argument", names);
  }
  // f(a...) once done() has passed: the a... are read (in any order) before either
  template <typename F, typename... A>
  auto then(F f, A... a) {
    done();
    return f(a...);
  }

 private:
  [[noreturn]] void fail(const char* what, const std::string& names) const {
    throw py::type_error(std::string(fn_) + ": " + what + " " + names);
  }
  [[noreturn]] void wrong_type(const char* k, const char* want, const py::handle& v) const {
    fail("argument", "'" + std::string(k) + "' must be " + want + ", got " + Py_TYPE(v.ptr())->tp_name);
  }

  // the interned str of a key name, made once per name: a lookup costs neither a new str nor its hash
  static PyObject* key(const char* k) {
    static std::unordered_map<std::string, PyObject*> keys;
    PyObject*& o = keys[k];
    if (!o && !(o = PyUnicode_InternFromString(k))) throw py::error_already_set();
    return o;
  }

  py::object take(const char* k) {
    py::object v = py::reinterpret_borrow<py::object>(PyDict_GetItemWithError(d_.ptr(), key(k)));
    if (v) PyDict_DelItem(d_.ptr(), key(k));
    else if (PyErr_Occurred()) throw py::error_already_set();
    else fail("missing argument", "'" + std::string(k) + "'");
    return v;
  }

  template <typename T>
  T get(const char* k, const char* want) {
    py::object v = take(k);
    try {
      return v.cast<T>();
    } catch (const py::cast_error&) {
      wrong_type(k, want, v);
    }
  }

  const char* fn_;
  py::dict d_;
};

// The common entry point: one struct from its fill function, then k(&struct, [args[grid],] stream);
// with three builds of k, args["prec"] selects one first.
template <typename A, typename S>
int launch(Args& x, A (*fill)(Args&), int (*k)(const A*, S)) {
  const A a = fill(x);
  return x.then(k, &a, (S)x.u("stream"));
}
template <typename A, typename S>
int launch(Args& x, A (*fill)(Args&), const char* grid, int (*k)(const A*, int, S)) {
  const A a = fill(x);
  return x.then(k, &a, x.i(grid), (S)x.u("stream"));
}
template <typename A, typename S>
int launch(Args& x, A (*fill)(Args&), const char* grid, int (*k)(const A*, int, S), decltype(k) k_f16, decltype(k) k_x3) {
  return launch(x, fill, grid, by_prec(x.i("prec"), k, k_f16, k_x3));
}
// m.name(**kwargs) = launch(Args(kwargs), l...)
template <typename... L>
void def_launch(py::module& m, const char* name, L... l) {
  m.def(name, [=](py::kwargs kw) { Args x(name, kw); return launch(x, l...); });
}
