// fastcall.cpp -- colosseumrl_amd._crl_fast: the two calls of a rollout region as CPython C-API functions.
//
// A 20-step rollout launch of 65,536 games is ~19 us of kernel inside a ~31 us region, and the GPU idles while the host
// prepares the call.  ctypes marshals every argument of a foreign call through converter objects: 0.71 us for the rollout
// entry's twelve arguments (one a ten-pointer struct by value) before anything is launched, 0.27 us for the four scalars
// that are left once the constant arguments are bound into a launch plan (include/colosseum_hip.h, crl_rollout_launch), and
// 0.08 us for those four through a METH_FASTCALL function (warm; tools/debug/host_latency.py, docs/history.md -- the first
// region of a process, which the benchmark times, gains 2.6 us).  Nothing here touches HIP: both functions call the C ABI
// of libcolosseum_hip.so, release the GIL around the call as ctypes does (the wait may spin for a whole long rollout), and
// hand the library's return code back -- the Python side raises through crl_last_error, which is thread-local and still
// holds the message then.
#define PY_SSIZE_T_CLEAN
#include <Python.h>
#include <stdint.h>
#include "../../include/colosseum_hip.h"

namespace {

// an integer argument as 64 bits, masked (a 64-bit seed or a handle above 2^63 survives; negative values wrap as in C).
// An int, or off the fast path anything with __index__ (a numpy integer); a float or None is a TypeError.
bool as_u64(PyObject *o, const char *name, uint64_t &out)
{
    if (PyLong_Check(o)) {
        out = (uint64_t)PyLong_AsUnsignedLongLongMask(o);
        return !(out == (uint64_t)-1 && PyErr_Occurred());
    }
    PyObject *i = PyIndex_Check(o) ? PyNumber_Index(o) : nullptr;
    if (!i) {
        if (!PyErr_Occurred()) PyErr_Format(PyExc_TypeError, "%s must be an int, not %.200s", name, Py_TYPE(o)->tp_name);
        return false;
    }
    out = (uint64_t)PyLong_AsUnsignedLongLongMask(i);
    Py_DECREF(i);
    return !(out == (uint64_t)-1 && PyErr_Occurred());
}

bool arity(const char *fn, const Py_ssize_t got, const Py_ssize_t want)
{
    if (got == want) return true;
    PyErr_Format(PyExc_TypeError, "%s takes exactly %zd arguments (%zd given)", fn, want, got);
    return false;
}

// rollout_launch(plan, seed, T, stream) -> rc
PyObject *rollout_launch(PyObject *, PyObject *const *args, Py_ssize_t nargs)
{
    uint64_t plan, seed, stream;
    if (!arity("rollout_launch", nargs, 4)) return nullptr;
    if (!as_u64(args[0], "plan", plan) || !as_u64(args[1], "seed", seed) || !as_u64(args[3], "stream", stream)) return nullptr;
    if (!PyLong_Check(args[2])) {
        PyErr_Format(PyExc_TypeError, "T must be an int, not %.200s", Py_TYPE(args[2])->tp_name);
        return nullptr;
    }
    const long T = PyLong_AsLong(args[2]);
    if (T == -1 && PyErr_Occurred()) return nullptr;
    if (T < INT32_MIN || T > INT32_MAX) {
        PyErr_SetString(PyExc_OverflowError, "T does not fit a C int");
        return nullptr;
    }
    int rc;
    Py_BEGIN_ALLOW_THREADS
    rc = crl_rollout_launch((const crl_plan *)(uintptr_t)plan, seed, (int)T, (void *)(uintptr_t)stream);
    Py_END_ALLOW_THREADS
    return PyLong_FromLong(rc);
}

// stream_wait_mapped(stream, flag_device, flag_host, seq, timeout_s) -> rc
PyObject *stream_wait_mapped(PyObject *, PyObject *const *args, Py_ssize_t nargs)
{
    uint64_t stream, flag_device, flag_host, seq;
    if (!arity("stream_wait_mapped", nargs, 5)) return nullptr;
    if (!as_u64(args[0], "stream", stream) || !as_u64(args[1], "flag_device", flag_device) ||
        !as_u64(args[2], "flag_host", flag_host) || !as_u64(args[3], "seq", seq))
        return nullptr;
    if (!PyFloat_Check(args[4]) && !PyLong_Check(args[4])) {
        PyErr_Format(PyExc_TypeError, "timeout_s must be a number, not %.200s", Py_TYPE(args[4])->tp_name);
        return nullptr;
    }
    const double timeout_s = PyFloat_AsDouble(args[4]);
    if (timeout_s == -1.0 && PyErr_Occurred()) return nullptr;
    int rc;
    Py_BEGIN_ALLOW_THREADS
    rc = crl_stream_wait_mapped((void *)(uintptr_t)stream, (uint32_t *)(uintptr_t)flag_device,
                                (const volatile uint32_t *)(uintptr_t)flag_host, (uint32_t)seq, timeout_s);
    Py_END_ALLOW_THREADS
    return PyLong_FromLong(rc);
}

PyMethodDef methods[] = {
    {"rollout_launch", (PyCFunction)(void (*)(void))rollout_launch, METH_FASTCALL,
     "rollout_launch(plan, seed, T, stream) -> rc: crl_rollout_launch on a plan of crl_*_rollout_bind (handles as ints)"},
    {"stream_wait_mapped", (PyCFunction)(void (*)(void))stream_wait_mapped, METH_FASTCALL,
     "stream_wait_mapped(stream, flag_device, flag_host, seq, timeout_s) -> rc: crl_stream_wait_mapped (addresses as ints)"},
    {nullptr, nullptr, 0, nullptr}};

PyModuleDef module = {PyModuleDef_HEAD_INIT, "_crl_fast",
                      "METH_FASTCALL entries of the two calls of a rollout region (csrc/fastcall.cpp); see colosseumrl_amd._native.fast()",
                      -1, methods, nullptr, nullptr, nullptr, nullptr};

} // namespace

PyMODINIT_FUNC PyInit__crl_fast(void)
{
    PyObject *m = PyModule_Create(&module);
    if (m && PyModule_AddIntConstant(m, "ABI_VERSION", CRL_ABI_VERSION) < 0) {
        Py_DECREF(m);
        return nullptr;
    }
    return m;
}
