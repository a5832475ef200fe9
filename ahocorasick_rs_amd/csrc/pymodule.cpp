// pymodule.cpp -- C++ CPython extension `ahocorasick_rs_amd.ahocorasick_rs`.
//
// Host-side mirror of the reference's PyO3 module (/root/reference/src/lib.rs):
// same classes, signatures, defaults, keyword names and exceptions, sitting on
// the C ABI of include/acx.h instead of the `aho-corasick` crate.  The
// reference's host is Rust; Rust is not available in this image, so the shim is
// C++ (raw CPython C API).  Reference lines are cited at each entry point.
//
//   #[pymodule] fn ahocorasick_rs          src/lib.rs:438-445
//   class MatchKind / Implementation       src/lib.rs:92-128
//   class AhoCorasick                      src/lib.rs:29-33, 131-273
//   class BytesAhoCorasick                 src/lib.rs:360-435
#define PY_SSIZE_T_CLEAN
#include <Python.h>

#include <cstdint>
#include <cstring>
#include <iterator>
#include <map>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>

#include "acx.h"

namespace {

// ---------------------------------------------------------------------------
// enums: MatchKind, Implementation  (pyclass(eq) simple enums)
// ---------------------------------------------------------------------------
struct EnumObject {
    PyObject_HEAD
    int value;
    const char *qualname; // e.g. "MatchKind.Standard"
};

PyTypeObject *MatchKindType = nullptr;
PyTypeObject *ImplementationType = nullptr;

PyObject *enum_repr(PyObject *self) {
    return PyUnicode_FromString(reinterpret_cast<EnumObject *>(self)->qualname);
}
Py_hash_t enum_hash(PyObject *self) { return reinterpret_cast<EnumObject *>(self)->value + 1; }
PyObject *enum_int(PyObject *self) {
    return PyLong_FromLong(reinterpret_cast<EnumObject *>(self)->value);
}
PyObject *enum_richcompare(PyObject *a, PyObject *b, int op) {
    if (op != Py_EQ && op != Py_NE) Py_RETURN_NOTIMPLEMENTED;
    int eq;
    // pyclass(eq) without eq_int (src/lib.rs:93, 113): only members of the same enum compare
    // equal; `MatchKind.Standard == 0` is False
    if (Py_TYPE(a) != Py_TYPE(b)) Py_RETURN_NOTIMPLEMENTED;
    eq = reinterpret_cast<EnumObject *>(a)->value == reinterpret_cast<EnumObject *>(b)->value;
    if ((op == Py_EQ) == (eq != 0)) Py_RETURN_TRUE;
    Py_RETURN_FALSE;
}

PyType_Slot enum_slots[] = {
    {Py_tp_repr, reinterpret_cast<void *>(enum_repr)},
    {Py_tp_hash, reinterpret_cast<void *>(enum_hash)},
    {Py_tp_richcompare, reinterpret_cast<void *>(enum_richcompare)},
    {Py_nb_int, reinterpret_cast<void *>(enum_int)},
    {Py_nb_index, reinterpret_cast<void *>(enum_int)},
    {0, nullptr},
};

// `full` must outlive the type (CPython keeps the pointer as tp_name)
PyTypeObject *make_enum(PyObject *module, const char *name, const char *full,
                        const char *const *variants, const char *const *qualnames, int n) {
    PyType_Spec spec = {full, sizeof(EnumObject), 0,
                        Py_TPFLAGS_DEFAULT | Py_TPFLAGS_DISALLOW_INSTANTIATION, enum_slots};
    PyTypeObject *tp = reinterpret_cast<PyTypeObject *>(PyType_FromSpec(&spec));
    if (!tp) return nullptr;
    for (int i = 0; i < n; i++) {
        EnumObject *o = PyObject_New(EnumObject, tp);
        if (!o) return nullptr;
        o->value = i;
        o->qualname = qualnames[i];
        if (PyObject_SetAttrString(reinterpret_cast<PyObject *>(tp), variants[i],
                                   reinterpret_cast<PyObject *>(o)) < 0)
            return nullptr;
        Py_DECREF(o);
    }
    // no public constructor
    if (PyModule_AddObject(module, name, reinterpret_cast<PyObject *>(tp)) < 0) return nullptr;
    Py_INCREF(tp);
    return tp;
}

// ---------------------------------------------------------------------------
// helpers
// ---------------------------------------------------------------------------
// status code -> Python exception (SURVEY.md §8b "Errors")
PyObject *raise_acx(int rc) {
    const char *msg = acx_last_error();
    switch (rc) {
    case ACX_EINVAL: case ACX_EEMPTY: case ACX_EOVERLAP: case ACX_ETOOBIG:
        PyErr_SetString(PyExc_ValueError, msg); break; // src/lib.rs:36-39, 215, 406
    case ACX_ENOMEM: PyErr_SetString(PyExc_MemoryError, msg); break;
    default: PyErr_SetString(PyExc_RuntimeError, msg); break; // no device / HIP failure
    }
    return nullptr;
}

// `overlapping: bool` / `store_patterns: Option<bool>` (src/lib.rs:135, 229, 253, 422): PyO3
// extracts a real bool and raises TypeError for anything else
bool parse_bool(PyObject *o, const char *name, int *out) {
    if (!PyBool_Check(o)) {
        PyErr_Format(PyExc_TypeError, "argument '%s': '%.100s' object cannot be converted to 'PyBool'", name,
                     Py_TYPE(o)->tp_name);
        return false;
    }
    *out = o == Py_True;
    return true;
}

bool parse_matchkind(PyObject *o, int *out) {
    if (!o) { *out = ACX_MATCH_STANDARD; return true; }
    if (Py_TYPE(o) != MatchKindType) {
        PyErr_Format(PyExc_TypeError, "argument 'matchkind': '%.100s' object cannot be converted to 'MatchKind'",
                     Py_TYPE(o)->tp_name);
        return false;
    }
    *out = reinterpret_cast<EnumObject *>(o)->value;
    return true;
}

bool parse_implementation(PyObject *o, int *out) {
    if (!o || o == Py_None) { *out = ACX_IMPL_AUTO; return true; }
    if (Py_TYPE(o) != ImplementationType) {
        PyErr_Format(PyExc_TypeError,
                     "argument 'implementation': '%.100s' object cannot be converted to 'Implementation'",
                     Py_TYPE(o)->tp_name);
        return false;
    }
    *out = reinterpret_cast<EnumObject *>(o)->value;
    return true;
}

// PyBufferBytes::try_from, src/lib.rs:282-302
bool get_bytes_view(PyObject *obj, Py_buffer *view) {
    if (PyObject_GetBuffer(obj, view, PyBUF_FULL_RO) < 0) return false; // TypeError for non-buffers
    if (view->ndim > 1) {
        PyBuffer_Release(view);
        PyErr_SetString(PyExc_TypeError, "Only one-dimensional sequences are supported");
        return false;
    }
    // PyBuffer::<u8>::get (src/lib.rs:286) accepts unsigned one-byte items only: format "B"
    // (absent = "B"), optionally behind a byte-order character; 'b', 'c', '?' are rejected
    const char *fmt = view->format;
    if (fmt && (*fmt == '@' || *fmt == '=' || *fmt == '<' || *fmt == '>' || *fmt == '!')) fmt++;
    if (view->itemsize != 1 || (fmt && !(fmt[0] == 'B' && fmt[1] == 0))) {
        PyBuffer_Release(view);
        PyErr_SetString(PyExc_BufferError, "buffer contents are not compatible with u8");
        return false;
    }
    if (!PyBuffer_IsContiguous(view, 'C')) {
        PyBuffer_Release(view);
        PyErr_SetString(PyExc_TypeError, "Must be a contiguous sequence of bytes");
        return false;
    }
    return true;
}

PyObject *matches_to_list(const acx_match_t *m, uint64_t n) {
    PyObject *list = PyList_New((Py_ssize_t)n);
    if (!list) return nullptr;
    for (uint64_t i = 0; i < n; i++) {
        PyObject *t = PyTuple_New(3);
        if (!t) { Py_DECREF(list); return nullptr; }
        PyObject *a = PyLong_FromUnsignedLongLong(m[i].pattern);
        PyObject *b = PyLong_FromUnsignedLongLong(m[i].start);
        PyObject *c = PyLong_FromUnsignedLongLong(m[i].end);
        if (!a || !b || !c) { Py_XDECREF(a); Py_XDECREF(b); Py_XDECREF(c); Py_DECREF(t); Py_DECREF(list); return nullptr; }
        PyTuple_SET_ITEM(t, 0, a); PyTuple_SET_ITEM(t, 1, b); PyTuple_SET_ITEM(t, 2, c);
        PyList_SET_ITEM(list, (Py_ssize_t)i, t);
    }
    return list;
}

// f() with the GIL released (py.detach, src/lib.rs:238, 261, 433)
template <typename F> int nogil(F &&f) {
    int rc;
    Py_BEGIN_ALLOW_THREADS
    rc = f();
    Py_END_ALLOW_THREADS
    return rc;
}

// An int argument: a real int, no bool (TypeError, naming the argument).  overflow: -1 / 0 / +1 as the value lies below, in or
// above int64 (*out is then -1); the range and its message are the caller's.  A caller without a rule for that passes none and
// gets CPython's own OverflowError.
bool parse_int(PyObject *o, const char *name, long long *out, int *overflow = nullptr) {
    if (!PyLong_Check(o) || PyBool_Check(o)) {
        PyErr_Format(PyExc_TypeError, "argument '%s': '%.100s' object cannot be converted to 'PyInt'", name, Py_TYPE(o)->tp_name);
        return false;
    }
    int of = 0;
    *out = PyLong_AsLongLongAndOverflow(o, &of);
    if (*out == -1 && !of && PyErr_Occurred()) return false;
    if (overflow) *overflow = of;
    else if (of) { PyLong_AsLongLong(o); return false; } // (raises it)
    return true;
}

// gap / context: an int 0 .. 2^63 - 1; sets the exception
bool parse_u63(PyObject *o, const char *name, uint64_t *out) {
    long long v;
    int overflow;
    if (!parse_int(o, name, &v, &overflow)) return false;
    if (overflow || v < 0) {
        PyErr_Format(PyExc_ValueError, "%s must be in range(2**63)", name);
        return false;
    }
    *out = (uint64_t)v;
    return true;
}

// the items item(b) .. item(e - 1) as a list; nullptr (and the list dropped) when an item cannot be made
template <typename Item> PyObject *list_of(uint64_t b, uint64_t e, Item &&item) {
    PyObject *list = PyList_New((Py_ssize_t)(e - b));
    for (uint64_t i = b; list && i < e; i++) {
        PyObject *x = item(i);
        if (!x) { Py_CLEAR(list); break; }
        PyList_SET_ITEM(list, (Py_ssize_t)(i - b), x);
    }
    return list;
}

// ... cut into one list per row by the rows' offsets (ro: rows + 1 entries), or, ro = null, the n items as one list
template <typename Item> PyObject *rows_of(const std::vector<int64_t> *ro, uint64_t n, Item &&item) {
    if (!ro) return list_of(0, n, item);
    return list_of(0, ro->size() - 1, [&](uint64_t h) { return list_of((uint64_t)(*ro)[h], (uint64_t)(*ro)[h + 1], item); });
}

// item i of a blob cut by offsets: bytes, or (utf8) the decoded str
PyObject *cut_item(const std::vector<uint8_t> &data, const std::vector<int64_t> &off, uint64_t i, bool utf8) {
    const char *p = reinterpret_cast<const char *>(data.data()) + off[(size_t)i];
    const Py_ssize_t n = (Py_ssize_t)(off[(size_t)i + 1] - off[(size_t)i]);
    return utf8 ? PyUnicode_DecodeUTF8(p, n, nullptr) : PyBytes_FromStringAndSize(p, n);
}

PyObject *info_dict(acx_automaton_t *a) {
    acx_info_t i;
    if (acx_automaton_info(a, &i) != ACX_OK) return raise_acx(ACX_EINVAL);
    return Py_BuildValue("{s:K,s:K,s:I,s:I,s:I,s:I,s:K,s:I,s:s,s:i,s:i,s:I,s:O}", "n_patterns",
                         (unsigned long long)i.n_patterns, "n_states", (unsigned long long)i.n_states,
                         "n_classes", i.n_classes, "stride", i.stride, "min_pattern_len",
                         i.min_pattern_len, "max_pattern_len", i.max_pattern_len, "table_bytes",
                         (unsigned long long)i.table_bytes, "lds_hot_rows", i.lds_hot_rows, "kernel",
                         i.kernel == ACX_KERNEL_PREFILTER ? "prefilter" : "dfa_walk", "match_kind",
                         i.match_kind, "device", i.device, "filter_q", i.filter_q, "ascii_case_insensitive",
                         (i.flags & ACX_BUILD_ASCII_CASE_INSENSITIVE) ? Py_True : Py_False);
}

// Replicas of an object's automaton on other devices (find_matches_as_indexes_batch(devices=[...])):
// built on first use, owned by the Python object.
typedef std::map<int, acx_automaton_t *> Replicas;

void free_replicas(Replicas *r) {
    if (!r) return;
    for (auto &kv : *r) acx_free_automaton(kv.second);
    delete r;
}

// devices (None, or a sequence of device ordinals) -> the handles the batch is sharded over
bool batch_handles(acx_automaton_t *a, PyObject *devices, Replicas **replicas, std::vector<acx_automaton_t *> *out) {
    out->clear();
    if (!devices || devices == Py_None) { out->push_back(a); return true; }
    PyObject *seq = PySequence_Fast(devices, "devices must be a sequence of device ordinals");
    if (!seq) return false;
    const Py_ssize_t n = PySequence_Fast_GET_SIZE(seq);
    if (n == 0) {
        Py_DECREF(seq);
        PyErr_SetString(PyExc_ValueError, "devices must name at least one device");
        return false;
    }
    for (Py_ssize_t i = 0; i < n; i++) {
        const long d = PyLong_AsLong(PySequence_Fast_GET_ITEM(seq, i));
        if (d == -1 && PyErr_Occurred()) { Py_DECREF(seq); return false; }
        if (d == acx_automaton_device(a)) { out->push_back(a); continue; }
        if (!*replicas) *replicas = new Replicas();
        auto it = (*replicas)->find((int)d);
        if (it == (*replicas)->end()) {
            acx_automaton_t *r = nullptr;
            const int rc = acx_replicate(a, (int)d, &r);
            if (rc != ACX_OK) { Py_DECREF(seq); raise_acx(rc); return false; }
            it = (*replicas)->emplace((int)d, r).first;
        }
        out->push_back(it->second);
    }
    Py_DECREF(seq);
    return true;
}

// The haystacks of a _batch method: a sequence of str (utf8, as UTF-8) or buffers, back to back in one blob with n + 1
// offsets and a trailing 0 byte (the blob of an empty batch still has an address).  named: a str class's TypeError names the
// argument, as `haystack` does in the single forms (the summaries, replace_all_batch); else it is PyO3's for a list item.
struct Packed {
    std::vector<uint8_t> blob;
    std::vector<uint64_t> off;
    bool all_ascii = true;
    Py_ssize_t n = 0;
};

bool pack_sequence(PyObject *haystacks, bool utf8, bool named, Packed *out) {
    PyObject *seq = PySequence_Fast(haystacks, "haystacks must be a sequence");
    if (!seq) return false;
    out->n = PySequence_Fast_GET_SIZE(seq);
    out->off.assign((size_t)out->n + 1, 0);
    for (Py_ssize_t i = 0; i < out->n; i++) {
        PyObject *it = PySequence_Fast_GET_ITEM(seq, i);
        if (utf8) {
            if (!PyUnicode_Check(it)) {
                PyErr_Format(PyExc_TypeError, named ? "argument 'haystack': '%.100s' object cannot be converted to 'PyString'"
                                                    : "'%.100s' object cannot be converted to 'PyString'", Py_TYPE(it)->tp_name);
                Py_DECREF(seq); return false;
            }
            Py_ssize_t len; const char *s = PyUnicode_AsUTF8AndSize(it, &len);
            if (!s) { Py_DECREF(seq); return false; }
            out->all_ascii = out->all_ascii && PyUnicode_IS_ASCII(it);
            out->blob.insert(out->blob.end(), s, s + len);
        } else {
            Py_buffer v;
            if (!get_bytes_view(it, &v)) { Py_DECREF(seq); return false; }
            out->blob.insert(out->blob.end(), (const uint8_t *)v.buf, (const uint8_t *)v.buf + v.len);
            PyBuffer_Release(&v);
        }
        out->off[(size_t)i + 1] = out->blob.size();
    }
    Py_DECREF(seq);
    out->blob.push_back(0);
    return true;
}

// One entry per CHARACTER of a str haystack.  row: what the library made of hay's UTF-8 bytes, one entry per byte.  text: the
// entries of a covered character's continuation bytes are dropped (fill is ASCII, so a continuation byte that differs from
// the haystack's is a covered one) and the rest is decoded; else (the 0 / 1 mask) the entry of every continuation byte is.
PyObject *per_character(const uint8_t *hay, const uint8_t *row, size_t len, bool text) {
    std::string s;
    s.reserve(len);
    for (size_t i = 0; i < len; i++) {
        const bool cont = (hay[i] & 0xC0) == 0x80;
        if (cont && (!text || row[i] != hay[i])) continue;
        s.push_back((char)row[i]);
    }
    return text ? PyUnicode_DecodeUTF8(s.data(), (Py_ssize_t)s.size(), nullptr) : PyBytes_FromStringAndSize(s.data(), (Py_ssize_t)s.size());
}

// ---------------------------------------------------------------------------
// The two automaton classes.  Both begin alike, so a method that both have is ONE function: it takes the automaton from the
// base and asks the object whether it is the str class.
// ---------------------------------------------------------------------------
struct AutomatonObject {
    PyObject_HEAD
    acx_automaton_t *ac;
    Replicas *replicas; // automata on other devices (batch calls with devices=[...]), or NULL
};
struct AcObject : AutomatonObject { // AhoCorasick (str)
    PyObject *patterns; // list[str] or NULL   (src/lib.rs:30-33 `patterns: Option<Vec<Py<PyString>>>`)
};
typedef AutomatonObject BacObject;  // BytesAhoCorasick

PyTypeObject *AhoCorasickType = nullptr;
acx_automaton_t *ac_of(PyObject *self) { return reinterpret_cast<AutomatonObject *>(self)->ac; }
bool utf8_of(PyObject *self) { return Py_TYPE(self) == AhoCorasickType; } // the str class: haystacks are str, searched as UTF-8

void automaton_dealloc(PyObject *self) {
    AutomatonObject *o = reinterpret_cast<AutomatonObject *>(self);
    if (o->ac) acx_free_automaton(o->ac);
    free_replicas(o->replicas);
    if (utf8_of(self)) Py_XDECREF(static_cast<AcObject *>(o)->patterns);
    PyTypeObject *tp = Py_TYPE(self);
    tp->tp_free(self);
    Py_DECREF(tp);
}

// the packed patterns -> a new object of `type`, or the build's error (the reference yields the GIL while building,
// src/lib.rs:198)
AutomatonObject *new_automaton(PyTypeObject *type, std::vector<uint8_t> &blob, const std::vector<uint64_t> &off, int mk, int impl, int ci) {
    acx_automaton_t *ac = nullptr;
    blob.push_back(0);
    const int rc = nogil([&] { return acx_build_ex(blob.data(), off.data(), off.size() - 1, mk, impl, ci ? ACX_BUILD_ASCII_CASE_INSENSITIVE : 0, &ac); });
    if (rc != ACX_OK) { raise_acx(rc); return nullptr; }
    AutomatonObject *self = reinterpret_cast<AutomatonObject *>(type->tp_alloc(type, 0));
    if (!self) { acx_free_automaton(ac); return nullptr; }
    self->ac = ac;
    self->replicas = nullptr;
    return self;
}

// src/lib.rs:134-224
PyObject *ac_new(PyTypeObject *type, PyObject *args, PyObject *kwargs) {
    static const char *kw[] = {"patterns", "matchkind", "store_patterns", "implementation", "ascii_case_insensitive", nullptr};
    PyObject *patterns = nullptr, *mk_o = nullptr, *store_o = Py_None, *impl_o = Py_None, *ci_o = Py_False;
    if (!PyArg_ParseTupleAndKeywords(args, kwargs, "O|OOOO:AhoCorasick", const_cast<char **>(kw),
                                     &patterns, &mk_o, &store_o, &impl_o, &ci_o))
        return nullptr;
    int mk, impl, ci;
    if (!parse_matchkind(mk_o, &mk) || !parse_implementation(impl_o, &impl)) return nullptr;
    int store = -1; // None -> heuristic
    if (store_o != Py_None && !parse_bool(store_o, "store_patterns", &store)) return nullptr;
    // the crate's AhoCorasickBuilder::ascii_case_insensitive: a real bool, as store_patterns
    if (!parse_bool(ci_o, "ascii_case_insensitive", &ci)) return nullptr;
    PyObject *iter = PyObject_GetIter(patterns); // non-iterable -> TypeError (tests/test_ac.py:79-80)
    if (!iter) return nullptr;
    PyObject *kept = PyList_New(0);
    if (!kept) { Py_DECREF(iter); return nullptr; }
    std::vector<uint8_t> blob;
    std::vector<uint64_t> off(1, 0);
    uint64_t total_chars = 0;
    bool heuristic_store = true; // src/lib.rs:164-178: store while the running total <= 4096
    PyObject *item;
    bool failed = false;
    while ((item = PyIter_Next(iter))) {
        if (!PyUnicode_Check(item)) { // cast_into::<PyString>, src/lib.rs:147-150
            PyErr_Format(PyExc_TypeError, "'%.100s' object cannot be converted to 'PyString'",
                         Py_TYPE(item)->tp_name);
            Py_DECREF(item); failed = true; break;
        }
        Py_ssize_t len;
        const char *s = PyUnicode_AsUTF8AndSize(item, &len);
        if (!s) {
            // src/lib.rs:200: `extract::<PyBackedStr>().ok()` -> the reference silently stops
            // consuming patterns at a str that has no UTF-8 form (lone surrogates).
            PyErr_Clear();
            Py_DECREF(item);
            break;
        }
        if (len == 0) { // src/lib.rs:204-208
            PyErr_SetString(PyExc_ValueError, "You passed in an empty string as a pattern");
            Py_DECREF(item); failed = true; break;
        }
        blob.insert(blob.end(), s, s + len);
        off.push_back(blob.size());
        bool keep = store == 1;
        if (store == -1 && heuristic_store) {
            total_chars += (uint64_t)PyUnicode_GET_LENGTH(item);
            keep = true; // the reference pushes the pattern before testing the total
            if (total_chars > 4096) heuristic_store = false;
        }
        if (keep && PyList_Append(kept, item) < 0) { Py_DECREF(item); failed = true; break; }
        Py_DECREF(item);
    }
    Py_DECREF(iter);
    if (failed || PyErr_Occurred()) { Py_DECREF(kept); return nullptr; } // iterator errors propagate
    bool do_store = store == 1 || (store == -1 && heuristic_store);
    AcObject *self = static_cast<AcObject *>(new_automaton(type, blob, off, mk, impl, ci));
    if (self && do_store) self->patterns = kept;
    else Py_DECREF(kept);
    return reinterpret_cast<PyObject *>(self);
}

bool parse_find_args(PyObject *args, PyObject *kwargs, const char *fmt, PyObject **hay,
                     int *overlapping) {
    static const char *kw[] = {"haystack", "overlapping", nullptr};
    *overlapping = 0;
    PyObject *ov = nullptr;
    if (!PyArg_ParseTupleAndKeywords(args, kwargs, fmt, const_cast<char **>(kw), hay, &ov)) return false;
    return !ov || parse_bool(ov, "overlapping", overlapping);
}

bool str_view(PyObject *hay, const char **s, Py_ssize_t *len) {
    if (!PyUnicode_Check(hay)) {
        PyErr_Format(PyExc_TypeError, "argument 'haystack': '%.100s' object cannot be converted to 'PyString'",
                     Py_TYPE(hay)->tp_name);
        return false;
    }
    *s = PyUnicode_AsUTF8AndSize(hay, len);
    return *s != nullptr;
}

// ---------------------------------------------------------------------------
// replace_all (the crate's AhoCorasick::replace_all / replace_all_bytes; the reference binding stops at finding)
// ---------------------------------------------------------------------------
// replace_with -> blob + offsets (materialised once per call): str items as UTF-8 (utf8) or buffers
bool replacements(PyObject *replace_with, bool utf8, std::vector<uint8_t> *blob, std::vector<uint64_t> *off) {
    PyObject *iter = PyObject_GetIter(replace_with);
    if (!iter) return false;
    off->assign(1, 0);
    PyObject *item;
    while ((item = PyIter_Next(iter))) {
        if (utf8) {
            if (!PyUnicode_Check(item)) {
                PyErr_Format(PyExc_TypeError, "argument 'replace_with': '%.100s' object cannot be converted to 'PyString'",
                             Py_TYPE(item)->tp_name);
                Py_DECREF(item); Py_DECREF(iter); return false;
            }
            Py_ssize_t len;
            const char *s = PyUnicode_AsUTF8AndSize(item, &len);
            if (!s) { Py_DECREF(item); Py_DECREF(iter); return false; }
            blob->insert(blob->end(), s, s + len);
        } else {
            Py_buffer v;
            if (!get_bytes_view(item, &v)) { Py_DECREF(item); Py_DECREF(iter); return false; }
            blob->insert(blob->end(), (const uint8_t *)v.buf, (const uint8_t *)v.buf + v.len);
            PyBuffer_Release(&v);
        }
        off->push_back(blob->size());
        Py_DECREF(item);
    }
    Py_DECREF(iter);
    blob->push_back(0);
    return !PyErr_Occurred();
}

// a finished acx_replace -> bytes (allocated at its final size, the library copies straight into it) or, utf8, str.
// Frees r.  bounds != null: the haystacks' output offsets (n_hay + 1) are written there.
PyObject *replaced_result(acx_replaced_t *r, bool utf8, std::vector<uint64_t> *bounds = nullptr) {
    const uint64_t n = acx_replaced_len(r);
    if (bounds && acx_replaced_offsets(r, bounds->data()) != ACX_OK) { acx_free_replaced(r); return raise_acx(ACX_EINVAL); }
    PyObject *b = PyBytes_FromStringAndSize(nullptr, (Py_ssize_t)n);
    if (!b) { acx_free_replaced(r); return nullptr; }
    int rc;
    char *dst = PyBytes_AS_STRING(b);
    Py_BEGIN_ALLOW_THREADS
    rc = acx_replaced_copy(r, dst);
    acx_free_replaced(r);
    Py_END_ALLOW_THREADS
    if (rc != ACX_OK) { Py_DECREF(b); return raise_acx(rc); }
    if (!utf8) return b;
    PyObject *s = PyUnicode_DecodeUTF8(dst, (Py_ssize_t)n, "strict");
    Py_DECREF(b);
    return s;
}

// replace_all_batch: list[str] / list[bytes], [replace_all(h, replace_with) for h in haystacks]
PyObject *replace_all_batch(PyObject *self, PyObject *args, PyObject *kwargs) {
    static const char *kw[] = {"haystacks", "replace_with", nullptr};
    PyObject *haystacks, *replace_with;
    if (!PyArg_ParseTupleAndKeywords(args, kwargs, "OO:replace_all_batch", const_cast<char **>(kw), &haystacks, &replace_with)) return nullptr;
    acx_automaton_t *a = ac_of(self);
    const bool utf8 = utf8_of(self);
    Packed in;
    if (!pack_sequence(haystacks, utf8, true, &in)) return nullptr;
    const Py_ssize_t n = in.n;
    std::vector<uint8_t> blob;
    std::vector<uint64_t> off;
    if (!replacements(replace_with, utf8, &blob, &off)) return nullptr;
    acx_replaced_t *r = nullptr;
    const int rc = nogil([&] {
        return acx_replace(a, in.blob.data(), in.off[(size_t)n], in.off.data(), (uint64_t)n, blob.data(), off.data(), off.size() - 1, &r);
    });
    if (rc != ACX_OK) return raise_acx(rc);
    std::vector<uint64_t> bounds((size_t)n + 1, 0);
    PyObject *whole = replaced_result(r, false, &bounds);
    if (!whole) return nullptr;
    const char *w = PyBytes_AS_STRING(whole);
    PyObject *list = list_of(0, (uint64_t)n, [&](uint64_t i) {
        const char *p = w + bounds[(size_t)i];
        const Py_ssize_t len = (Py_ssize_t)(bounds[(size_t)i + 1] - bounds[(size_t)i]);
        return utf8 ? PyUnicode_DecodeUTF8(p, len, "strict") : PyBytes_FromStringAndSize(p, len);
    });
    Py_DECREF(whole);
    return list;
}

// find_matches_as_indexes_batch: list[list[tuple]].  devices: None = the object's own device; a sequence of ordinals = the
// batch is cut into that many contiguous ranges of haystacks, one host thread per device (acx_find_batch_multi).
PyObject *find_batch(PyObject *self, PyObject *args, PyObject *kwargs) {
    static const char *kw[] = {"haystacks", "overlapping", "devices", nullptr};
    PyObject *hs, *ov = nullptr, *devs = nullptr; int overlapping = 0;
    if (!PyArg_ParseTupleAndKeywords(args, kwargs, "O|OO:find_matches_as_indexes_batch",
                                     const_cast<char **>(kw), &hs, &ov, &devs))
        return nullptr;
    if (ov && !parse_bool(ov, "overlapping", &overlapping)) return nullptr;
    std::vector<acx_automaton_t *> handles;
    if (!batch_handles(ac_of(self), devs, &reinterpret_cast<AutomatonObject *>(self)->replicas, &handles)) return nullptr;
    Packed in;
    if (!pack_sequence(hs, utf8_of(self), false, &in)) return nullptr;
    std::vector<uint64_t> counts((size_t)in.n, 0);
    acx_match_t *m = nullptr; uint64_t total = 0;
    const int rc = nogil([&] {
        return acx_find_batch_multi(handles.data(), (int)handles.size(), in.blob.data(), in.off.data(), (uint64_t)in.n, overlapping,
                                    (utf8_of(self) && !in.all_ascii) ? 1 : 0, &m, &total, counts.data());
    });
    if (rc != ACX_OK) return raise_acx(rc);
    uint64_t pos = 0;
    PyObject *outer = list_of(0, (uint64_t)in.n, [&](uint64_t i) {
        PyObject *inner = matches_to_list(m + pos, counts[(size_t)i]);
        pos += counts[(size_t)i];
        return inner;
    });
    acx_free_matches(m);
    return outer;
}

PyObject *automaton_info(PyObject *self, PyObject *) { return info_dict(ac_of(self)); }

enum { SUM_IS_MATCH = 0, SUM_FIND_FIRST = 1, SUM_COUNT = 2, SUM_BY_PATTERN = 3 };

// src/lib.rs:369-413
PyObject *bac_new(PyTypeObject *type, PyObject *args, PyObject *kwargs) {
    static const char *kw[] = {"patterns", "matchkind", "implementation", "ascii_case_insensitive", nullptr};
    PyObject *patterns = nullptr, *mk_o = nullptr, *impl_o = Py_None, *ci_o = Py_False;
    if (!PyArg_ParseTupleAndKeywords(args, kwargs, "O|OOO:BytesAhoCorasick", const_cast<char **>(kw),
                                     &patterns, &mk_o, &impl_o, &ci_o))
        return nullptr;
    int mk, impl, ci;
    if (!parse_matchkind(mk_o, &mk) || !parse_implementation(impl_o, &impl)) return nullptr;
    if (!parse_bool(ci_o, "ascii_case_insensitive", &ci)) return nullptr;
    PyObject *iter = PyObject_GetIter(patterns);
    if (!iter) return nullptr;
    std::vector<uint8_t> blob;
    std::vector<uint64_t> off(1, 0);
    PyObject *item;
    bool failed = false;
    while ((item = PyIter_Next(iter))) {
        Py_buffer v;
        if (!get_bytes_view(item, &v)) { Py_DECREF(item); failed = true; break; }
        if (v.len == 0) { // src/lib.rs:386-389
            PyBuffer_Release(&v); Py_DECREF(item);
            PyErr_SetString(PyExc_ValueError, "You passed in an empty pattern");
            failed = true; break;
        }
        blob.insert(blob.end(), (const uint8_t *)v.buf, (const uint8_t *)v.buf + v.len);
        off.push_back(blob.size());
        PyBuffer_Release(&v); // no reference to the pattern objects is kept, src/lib.rs:350-351
        Py_DECREF(item);
    }
    Py_DECREF(iter);
    if (failed || PyErr_Occurred()) return nullptr;
    return reinterpret_cast<PyObject *>(new_automaton(type, blob, off, mk, impl, ci));
}

// ---- device-resident haystacks (extends the buffer adapter of src/lib.rs:276-340): an object that
// is no host buffer but exports __dlpack__ (a torch / cupy tensor in HBM) is searched where it lies
// -- no H2D copy.  DLPack structs (dlpack.h, ABI v0: the capsule "dltensor"):
struct DLDeviceC { int32_t device_type; int32_t device_id; };
struct DLDataTypeC { uint8_t code; uint8_t bits; uint16_t lanes; };
struct DLTensorC { void *data; DLDeviceC device; int32_t ndim; DLDataTypeC dtype; int64_t *shape; int64_t *strides; uint64_t byte_offset; };
struct DLManagedTensorC { DLTensorC dl_tensor; void *manager_ctx; void (*deleter)(DLManagedTensorC *); };
constexpr int32_t kDLCPU = 1, kDLCUDA = 2, kDLCUDAHost = 3, kDLROCM = 10, kDLROCMHost = 11;

// haystack -> (pointer, length, on_device).  Returns the capsule to release afterwards (new reference).  want_device < 0: a
// call without an automaton takes a tensor on any device.
PyObject *dlpack_view(PyObject *hay, int want_device, const uint8_t **ptr, uint64_t *len, bool *on_device) {
    PyObject *cap = PyObject_CallMethod(hay, "__dlpack__", nullptr);
    if (!cap) return nullptr;
    DLManagedTensorC *mt = PyCapsule_IsValid(cap, "dltensor")
                               ? static_cast<DLManagedTensorC *>(PyCapsule_GetPointer(cap, "dltensor")) : nullptr;
    if (!mt) {
        Py_DECREF(cap);
        PyErr_SetString(PyExc_TypeError, "__dlpack__ did not return a 'dltensor' capsule");
        return nullptr;
    }
    const DLTensorC &t = mt->dl_tensor;
    const char *err = nullptr;
    uint64_t n = 1;
    for (int32_t d = 0; d < t.ndim; d++) n *= (uint64_t)t.shape[d];
    if (t.ndim > 1) err = "Only one-dimensional sequences are supported";                  // src/lib.rs:288-292
    else if (t.dtype.code != 1 || t.dtype.bits != 8 || t.dtype.lanes != 1) err = "buffer contents are not compatible with u8";
    else if (t.ndim == 1 && t.strides && t.shape[0] > 1 && t.strides[0] != 1) err = "Must be a contiguous sequence of bytes"; // :293-297
    const bool dev = t.device.device_type == kDLROCM || t.device.device_type == kDLCUDA;
    const bool host = t.device.device_type == kDLCPU || t.device.device_type == kDLROCMHost ||
                      t.device.device_type == kDLCUDAHost;
    if (!err && !dev && !host) err = "unsupported DLPack device type";
    if (!err && dev && want_device >= 0 && t.device.device_id != want_device) {
        PyErr_Format(PyExc_ValueError, "haystack lives on device %d, the automaton on device %d",
                     (int)t.device.device_id, want_device);
        Py_DECREF(cap);
        return nullptr;
    }
    if (err) {
        PyErr_SetString(err[0] == 'b' ? PyExc_BufferError : PyExc_TypeError, err);
        Py_DECREF(cap);
        return nullptr;
    }
    *ptr = static_cast<const uint8_t *>(t.data) + t.byte_offset;
    *len = n;
    *on_device = dev;
    return cap;
}

void dlpack_release(PyObject *cap) { // we consumed the capsule: rename it and run the producer's deleter
    if (!cap) return;
    if (PyCapsule_IsValid(cap, "dltensor")) {
        DLManagedTensorC *mt = static_cast<DLManagedTensorC *>(PyCapsule_GetPointer(cap, "dltensor"));
        PyCapsule_SetName(cap, "used_dltensor");
        if (mt && mt->deleter) mt->deleter(mt);
    }
    Py_DECREF(cap);
}

// the tensor behind a capsule that dlpack_view returned
const DLTensorC &capsule_tensor(PyObject *cap) { return static_cast<DLManagedTensorC *>(PyCapsule_GetPointer(cap, "dltensor"))->dl_tensor; }

// The haystack of a single-haystack method: `len` bytes at `p`, in HBM (on_device) or in host memory.  It owns the Py_buffer
// or the capsule that keeps the bytes where they are, until it goes out of scope.
struct HaystackView {
    const uint8_t *p = nullptr;
    uint64_t len = 0;
    bool on_device = false;
    bool is_ascii = false; // a str without a character beyond ASCII: byte offsets are its character indexes
    Py_buffer buf;
    bool has_buf = false;
    PyObject *cap = nullptr;
    HaystackView() = default;
    HaystackView(const HaystackView &) = delete;
    HaystackView &operator=(const HaystackView &) = delete;
    ~HaystackView() { if (has_buf) PyBuffer_Release(&buf); dlpack_release(cap); }
};

// utf8 (the str class): a str, as its UTF-8 bytes.  Else a contiguous byte buffer or, tensors (the methods that take one): an
// object that is no buffer but exports __dlpack__ -- on want_device if it is in HBM (want_device < 0: on any).  Sets the
// exception.
bool haystack_view(PyObject *hay, bool utf8, bool tensors, int want_device, HaystackView *v) {
    if (utf8) {
        const char *s; Py_ssize_t len;
        if (!str_view(hay, &s, &len)) return false;
        v->p = reinterpret_cast<const uint8_t *>(s);
        v->len = (uint64_t)len;
        v->is_ascii = PyUnicode_IS_ASCII(hay);
        return true;
    }
    if (tensors && !PyObject_CheckBuffer(hay) && PyObject_HasAttrString(hay, "__dlpack__")) {
        v->cap = dlpack_view(hay, want_device, &v->p, &v->len, &v->on_device);
        return v->cap != nullptr;
    }
    if (!get_bytes_view(hay, &v->buf)) return false;
    v->has_buf = true;
    v->p = static_cast<const uint8_t *>(v->buf.buf);
    v->len = (uint64_t)v->buf.len;
    return true;
}

// One call on a HaystackView with the GIL released: host(p, len), or device(p, len) on a tensor in HBM -- behind everything
// queued on its device: the producer's kernels may still be writing the tensor on their own stream, and the library's
// streams are non-blocking ones.  device_ordinal: the tensor's (the automaton's: dlpack_view checked that).
template <typename Host, typename Device>
int single_dispatch(int device_ordinal, const HaystackView &v, Host &&host, Device &&device) {
    return nogil([&] {
        if (!v.on_device) return host(v.p, v.len);
        const int rc = acx_device_synchronize_on(device_ordinal);
        return rc == ACX_OK ? device(v.p, v.len) : rc;
    });
}

// ---------------------------------------------------------------------------
// summaries: is_match / find_first / count_matches / count_by_pattern and their batch forms (acx_summarize: the crate's
// AhoCorasick::is_match and ::find, and the counts of its iterators; the reference binding stops at the match list)
// ---------------------------------------------------------------------------
struct Summary {
    uint64_t total = 0;
    std::vector<uint64_t> counts, any, hist;
    std::vector<acx_match_t> first;
};

// one acx_summarize call (on_device: acx_summarize_device on a tensor in HBM) and the copies of the parts the method
// returns; the caller has released the GIL
int summarize(acx_automaton_t *a, const uint8_t *hay, uint64_t len, const uint64_t *offsets, uint64_t n_hay,
              bool on_device, int overlapping, int codepoints, int kind, bool batch, Summary *out) {
    const uint32_t what = kind == SUM_FIND_FIRST || (kind == SUM_IS_MATCH && batch) ? ACX_SUM_FIRST
                          : kind == SUM_BY_PATTERN ? ACX_SUM_BY_PATTERN : 0;
    acx_summary_t *r = nullptr;
    int rc = on_device ? acx_summarize_device(a, hay, len, nullptr, 0, 0, overlapping, codepoints, what, &r)
                       : acx_summarize(a, hay, len, offsets, n_hay, overlapping, codepoints, what, &r);
    if (rc == ACX_OK) {
        const uint64_t n = offsets ? n_hay : 1;
        out->total = acx_summary_total(r);
        if (kind == SUM_COUNT && batch) {
            out->counts.assign((size_t)n, 0);
            rc = acx_summary_counts(r, out->counts.data());
        } else if (kind == SUM_IS_MATCH && batch) {
            out->any.assign((size_t)((n + 63) / 64), 0);
            rc = acx_summary_any(r, out->any.data());
        } else if (kind == SUM_FIND_FIRST) {
            out->first.resize((size_t)n);
            rc = acx_summary_first(r, out->first.data());
        } else if (kind == SUM_BY_PATTERN) {
            acx_info_t info;
            rc = acx_automaton_info(a, &info);
            if (rc == ACX_OK) {
                out->hist.assign((size_t)info.n_patterns, 0);
                rc = acx_summary_by_pattern(r, out->hist.data());
            }
        }
    }
    acx_free_summary(r);
    return rc;
}

PyObject *first_to_object(const acx_match_t &m) {
    if (m.pattern == UINT64_MAX) Py_RETURN_NONE;
    return Py_BuildValue("(KKK)", (unsigned long long)m.pattern, (unsigned long long)m.start, (unsigned long long)m.end);
}

PyObject *u64_list(const std::vector<uint64_t> &v) {
    return list_of(0, v.size(), [&](uint64_t i) { return PyLong_FromUnsignedLongLong(v[(size_t)i]); });
}

PyObject *summary_to_object(const Summary &s, int kind, bool batch, Py_ssize_t n) {
    if (kind == SUM_BY_PATTERN) return u64_list(s.hist);
    if (!batch) {
        if (kind == SUM_IS_MATCH) return PyBool_FromLong(s.total != 0);
        if (kind == SUM_COUNT) return PyLong_FromUnsignedLongLong(s.total);
        return first_to_object(s.first[0]);
    }
    if (kind == SUM_COUNT) return u64_list(s.counts);
    return list_of(0, (uint64_t)n, [&](uint64_t i) {
        return kind == SUM_IS_MATCH ? PyBool_FromLong((long)((s.any[(size_t)i >> 6] >> (i & 63)) & 1)) : first_to_object(s.first[(size_t)i]);
    });
}

const char *const SUMMARY_FMT[2][4] = {{"O:is_match", "O:find_first", "O|O:count_matches", "O|O:count_by_pattern"},
                                       {"O:is_match_batch", "O:find_first_batch", "O|O:count_matches_batch",
                                        "O|O:count_by_pattern_batch"}};

// Every summary method: kind = SUM_IS_MATCH .. SUM_BY_PATTERN, batch: the *_batch form.  Code points are asked for only where
// offsets are returned (find_first) and the text is not ASCII; find_first is always a non-overlapping search.
template <int kind, bool batch> PyObject *summary(PyObject *self, PyObject *args, PyObject *kwargs) {
    acx_automaton_t *a = ac_of(self);
    const bool utf8 = utf8_of(self);
    // (is_match and find_first take no `overlapping`: the one does not depend on it, the other is the crate's find)
    const bool has_ov = kind == SUM_COUNT || kind == SUM_BY_PATTERN;
    const char *kw[] = {batch ? "haystacks" : "haystack", has_ov ? "overlapping" : nullptr, nullptr};
    PyObject *hay = nullptr, *ov = nullptr;
    int overlapping = 0;
    if (!PyArg_ParseTupleAndKeywords(args, kwargs, SUMMARY_FMT[batch][kind], const_cast<char **>(kw), &hay, &ov)) return nullptr;
    if (ov && !parse_bool(ov, "overlapping", &overlapping)) return nullptr;
    Summary s;
    int rc;
    Py_ssize_t n = 1;
    if (batch) {
        Packed in;
        if (!pack_sequence(hay, utf8, true, &in)) return nullptr;
        n = in.n;
        rc = nogil([&] {
            return summarize(a, in.blob.data(), in.off[(size_t)n], in.off.data(), (uint64_t)n, false, overlapping,
                             utf8 && !in.all_ascii && kind == SUM_FIND_FIRST, kind, true, &s);
        });
    } else {
        HaystackView v;
        if (!haystack_view(hay, utf8, true, acx_automaton_device(a), &v)) return nullptr;
        const int codepoints = utf8 && !v.is_ascii && kind == SUM_FIND_FIRST;
        rc = single_dispatch(
            acx_automaton_device(a), v,
            [&](const uint8_t *p, uint64_t len) { return summarize(a, p, len, nullptr, 0, false, overlapping, codepoints, kind, false, &s); },
            [&](const uint8_t *p, uint64_t len) { return summarize(a, p, len, nullptr, 0, true, overlapping, 0, kind, false, &s); }); // (reduced where it lies)
    }
    if (rc != ACX_OK) return raise_acx(rc);
    return summary_to_object(s, kind, batch, n);
}

// ---------------------------------------------------------------------------
// matches as columns: find_matches_as_columns / _batch -> MatchColumns (acx_find_columns / acx_find_columns_device).
// A MatchColumns owns the acx_columns_t; a Column is a view of one of its parts and keeps the MatchColumns alive; a DLPack
// capsule -- and whatever tensor a consumer makes of it -- keeps the Column alive until the consumer calls its deleter.
// ---------------------------------------------------------------------------
PyTypeObject *ColumnType = nullptr;

// What every result object -- the owner of a C ABI result and of the Columns made of its parts -- begins with.
struct ResultType;
struct OwnerObject {
    PyObject_HEAD
    const ResultType *rt;
    void *h;    // the C ABI's result
    int device; // the automaton's ordinal (where device parts lie)
};
struct MatchColumnsObject : OwnerObject {
    bool batch;
};
struct PatternCountsObject : OwnerObject {
    uint64_t n_patterns; // the matrix has this many columns
};
struct FilteredRowsObject : OwnerObject {
    uint64_t n_src;  // the rows of the batch that was filtered
    bool utf8;       // made by the str class: tolist() decodes
};
struct MatchSpansObject : OwnerObject {
    bool batch;
};
struct MatchSnippetsObject : OwnerObject {
    bool batch;
    bool utf8; // made by the str class: tolist() decodes
};
enum { TL_PATTERN = 0, TL_BEGIN = 1 };
struct TokenLabelsObject : OwnerObject {
    std::vector<int64_t> *row_offsets; // the sequence form: where every row's tokens begin (rows + 1 entries); else null
    // the device route: the capsules of the haystack, its offsets and the boundaries.  The call returns with the stage in
    // flight and its kernels read all three on the library's stream: the tensors stay the producer's until the result goes
    PyObject *inputs[3];
};
struct MatchesAtObject : OwnerObject {
    // the device route: the capsules of the haystack, its offsets and the positions.  The call returns with the walk in
    // flight and its kernels read all three on the library's stream: the tensors stay the producer's until the result goes
    PyObject *inputs[3];
};
struct SegmentsObject : OwnerObject {
    bool batch; // segment_batch: .row_offsets is a Column and tolist() gives one list per row
    // the device route: the capsules of the haystack and its offsets.  The call returns with the emitting kernels in flight
    // and they read both on the library's stream: the tensors stay the producer's until the result goes
    PyObject *inputs[3];
};
struct WordPiecesObject : OwnerObject {
    bool batch; // wordpiece_batch: .row_offsets is a Column and tolist() gives one list per row
    // where every row begins, for tolist()'s local positions -- one of three: the host routes' row begins in the result's
    // unit (rows + 1 entries), a row length, or the device offsets (inputs[1] keeps them alive)
    std::vector<int64_t> *row_begin;
    uint64_t row_length;
    const uint64_t *d_off;
    // the device route: the capsules of the haystack and its offsets.  The call returns with the emitting kernels in flight
    // and they read both on the library's stream: the tensors stay the producer's until the result goes
    PyObject *inputs[3];
};
enum { MR_OFFSETS = 0, MR_DATA = 1 };
struct MaskedRowsObject : OwnerObject {
    bool utf8;                 // made by the str class
    bool text;                 // mask_all_batch: the rows are the input's text; false: match_mask_batch, 0 / 1 bytes
    std::vector<uint8_t> *src; // a sequence of str with a non-ASCII one: its UTF-8 bytes, for tolist()'s entry per character
};

// The three calls a Column makes on its owner's result, cast from the C ABI's typed ones (data: with or without `which`)
struct OwnerOps {
    int (*on_device)(const void *h);
    const void *(*data)(const void *h, int which); // (waits for the device work)
    void (*free)(void *h);
};
template <typename T, int (*OnDevice)(const T *), auto Data, void (*Free)(T *)> OwnerOps owner_ops() {
    return {[](const void *h) { return OnDevice(static_cast<const T *>(h)); },
            [](const void *h, int which) -> const void * {
                (void)which;
                if constexpr (std::is_invocable_v<decltype(Data), const T *, int>) return Data(static_cast<const T *>(h), which);
                else return Data(static_cast<const T *>(h));
            },
            [](void *h) { Free(static_cast<T *>(h)); }};
}

// One row of RESULT_TYPES (behind the tolist methods below): all that tells one result type from another.
constexpr uint64_t NO_PART = ~0ull;
struct ResultType {
    const char *name; // "ahocorasick_rs.<Name>"
    int size;         // of the object
    OwnerOps ops;
    // the entries of part `which` (*elem = 1: uint8 bytes, else int64 words), or NO_PART: the attribute is None
    uint64_t (*part_len)(const OwnerObject *o, int which, int *elem);
    Py_ssize_t (*len)(PyObject *self);
    PyObject *(*tolist)(PyObject *self, PyObject *);
    const char *tolist_doc, *doc;
    // the attributes; {name, nullptr, nullptr, doc, which}: a part, served as a Column by owner_get_part
    std::vector<PyGetSetDef> getset;
    void (*dealloc)(PyObject *self);
    PyTypeObject *type; // made by PyInit
    PyMethodDef methods[2];
};
enum { RT_MATCH_COLUMNS, RT_PATTERN_COUNTS, RT_FILTERED_ROWS, RT_ROW_SCORES, RT_MASKED_ROWS, RT_ROW_OFFSETS, RT_MATCH_SPANS, RT_MATCH_SNIPPETS, RT_TOKEN_LABELS, RT_MATCHES_AT, RT_SEGMENTS, RT_WORD_PIECES, RT_COUNT };
extern ResultType RESULT_TYPES[RT_COUNT];

OwnerObject *owner_of(PyObject *s) { return reinterpret_cast<OwnerObject *>(s); }
template <typename T> T *handle(PyObject *s) { return static_cast<T *>(owner_of(s)->h); }
template <typename T> const T *handle(const OwnerObject *o) { return static_cast<const T *>(o->h); }

// a new owner of type RESULT_TYPES[rt] around the result h; frees h when the object cannot be made
OwnerObject *new_owner(int rt, void *h, int device) {
    const ResultType &t = RESULT_TYPES[rt];
    OwnerObject *o = reinterpret_cast<OwnerObject *>(t.type->tp_alloc(t.type, 0));
    if (!o) { t.ops.free(h); return nullptr; }
    o->rt = &t;
    o->h = h;
    o->device = device;
    return o;
}

void owner_dealloc(PyObject *self) {
    OwnerObject *o = owner_of(self);
    if (o->h) o->rt->ops.free(o->h); // (waits for the device work if nobody has: microseconds to a millisecond)
    PyTypeObject *tp = Py_TYPE(self);
    tp->tp_free(self);
    Py_DECREF(tp);
}

PyObject *owner_get_device(PyObject *s, void *) {
    if (!owner_of(s)->rt->ops.on_device(owner_of(s)->h)) Py_RETURN_NONE;
    return PyLong_FromLong(owner_of(s)->device);
}


struct ColumnObject {
    PyObject_HEAD
    PyObject *owner;
    int which;
    int64_t len;
    int elem;        // 0: int64 words; 1: uint8 bytes (a FilteredRows' or a MaskedRows' data)
};

PyObject *new_column(PyObject *owner, int which, uint64_t len, int elem = 0) {
    ColumnObject *col = reinterpret_cast<ColumnObject *>(ColumnType->tp_alloc(ColumnType, 0));
    if (!col) return nullptr;
    Py_INCREF(owner);
    col->owner = owner;
    col->which = which;
    col->len = (int64_t)len;
    col->elem = elem;
    return reinterpret_cast<PyObject *>(col);
}

void col_dealloc(PyObject *self) {
    Py_XDECREF(reinterpret_cast<ColumnObject *>(self)->owner);
    PyTypeObject *tp = Py_TYPE(self);
    tp->tp_free(self);
    Py_DECREF(tp);
}

int col_device(ColumnObject *o) { return owner_of(o->owner)->device; }
bool col_on_device(ColumnObject *o) { return owner_of(o->owner)->rt->ops.on_device(owner_of(o->owner)->h) != 0; }

// the part's address once the device work is done (GIL released around the wait); sets the exception
const void *col_data(ColumnObject *o) {
    const void *p;
    Py_BEGIN_ALLOW_THREADS
    p = owner_of(o->owner)->rt->ops.data(owner_of(o->owner)->h, o->which);
    Py_END_ALLOW_THREADS
    if (!p) PyErr_SetString(PyExc_RuntimeError, "the column's device work failed");
    return p;
}

Py_ssize_t col_len(PyObject *s) { return (Py_ssize_t)reinterpret_cast<ColumnObject *>(s)->len; }

PyObject *col_dlpack_device(PyObject *self_, PyObject *) {
    if (!col_on_device(reinterpret_cast<ColumnObject *>(self_))) return Py_BuildValue("(ii)", (int)kDLCPU, 0);
    return Py_BuildValue("(ii)", (int)kDLROCM, col_device(reinterpret_cast<ColumnObject *>(self_)));
}

// what a capsule points at: the tensor, its shape and stride, and the reference that keeps the data alive
struct ColumnExport {
    DLManagedTensorC mt;
    int64_t shape[1], strides[1];
    PyObject *column;
};

void column_export_deleter(DLManagedTensorC *mt) { // (called by the consumer, from any thread, with or without the GIL)
    ColumnExport *e = static_cast<ColumnExport *>(mt->manager_ctx);
    if (Py_IsInitialized()) { // (a tensor that outlives the interpreter: its column goes with the process)
        const PyGILState_STATE g = PyGILState_Ensure();
        Py_DECREF(e->column);
        PyGILState_Release(g);
    }
    delete e;
}

void column_capsule_destructor(PyObject *cap) { // a capsule nobody consumed still owns the export
    if (!PyCapsule_IsValid(cap, "dltensor")) return;
    DLManagedTensorC *mt = static_cast<DLManagedTensorC *>(PyCapsule_GetPointer(cap, "dltensor"));
    if (mt && mt->deleter) mt->deleter(mt);
}

// __dlpack__(stream=None, **ignored): the split is waited for on the host before the capsule is made, so the data is
// finished for a consumer on any stream and `stream` needs no work
PyObject *col_dlpack(PyObject *self_, PyObject *args, PyObject *) {
    if (PyTuple_GET_SIZE(args) > 1) {
        PyErr_SetString(PyExc_TypeError, "__dlpack__ takes at most one positional argument (stream)");
        return nullptr;
    }
    ColumnObject *self = reinterpret_cast<ColumnObject *>(self_);
    const void *p = col_data(self);
    if (!p) return nullptr;
    ColumnExport *e = new (std::nothrow) ColumnExport();
    if (!e) return PyErr_NoMemory();
    e->shape[0] = self->len;
    e->strides[0] = 1;
    e->mt.dl_tensor.data = const_cast<void *>(p);
    e->mt.dl_tensor.device = col_on_device(self) ? DLDeviceC{kDLROCM, col_device(self)} : DLDeviceC{kDLCPU, 0};
    e->mt.dl_tensor.ndim = 1;
    e->mt.dl_tensor.dtype = self->elem ? DLDataTypeC{1 /* kDLUInt */, 8, 1} : DLDataTypeC{0 /* kDLInt */, 64, 1};
    e->mt.dl_tensor.shape = e->shape;
    e->mt.dl_tensor.strides = e->strides;
    e->mt.dl_tensor.byte_offset = 0;
    e->mt.manager_ctx = e;
    e->mt.deleter = column_export_deleter;
    e->column = self_;
    PyObject *cap = PyCapsule_New(&e->mt, "dltensor", column_capsule_destructor);
    if (!cap) { delete e; return nullptr; }
    Py_INCREF(self_);
    return cap;
}

// the buffer protocol of a host column: read-only, format "q" (a FilteredRows' data: "B")
int col_getbuffer(PyObject *self_, Py_buffer *view, int flags) {
    ColumnObject *self = reinterpret_cast<ColumnObject *>(self_);
    view->obj = nullptr;
    if (col_on_device(self)) {
        PyErr_SetString(PyExc_BufferError, "the column is in device memory: use __dlpack__");
        return -1;
    }
    if (flags & PyBUF_WRITABLE) {
        PyErr_SetString(PyExc_BufferError, "the column is read-only");
        return -1;
    }
    const void *p = col_data(self);
    if (!p) return -1;
    static Py_ssize_t word_stride = 8, byte_stride = 1;
    const Py_ssize_t item = self->elem ? 1 : 8;
    view->buf = const_cast<void *>(p);
    view->len = (Py_ssize_t)self->len * item;
    view->itemsize = item;
    view->readonly = 1;
    view->ndim = 1;
    view->format = (flags & PyBUF_FORMAT) ? const_cast<char *>(self->elem ? "B" : "q") : nullptr;
    view->shape = (flags & PyBUF_ND) ? reinterpret_cast<Py_ssize_t *>(&self->len) : nullptr;
    view->strides = (flags & PyBUF_STRIDES) == PyBUF_STRIDES ? (self->elem ? &byte_stride : &word_stride) : nullptr;
    view->suboffsets = nullptr;
    view->internal = nullptr;
    Py_INCREF(self_);
    view->obj = self_;
    return 0;
}

PyMethodDef col_methods[] = {
    {"__dlpack__", reinterpret_cast<PyCFunction>(reinterpret_cast<void (*)()>(col_dlpack)), METH_VARARGS | METH_KEYWORDS,
     "__dlpack__(stream=None, **ignored) -> a 'dltensor' capsule of the column: 1-D, int64, contiguous.  Waits for the split "
     "kernel first: the data is finished for a consumer on any stream.  The capsule, and the tensor made of it, keep the "
     "result alive."},
    {"__dlpack_device__", col_dlpack_device, METH_NOARGS, "(kDLCPU, 0) or (kDLROCM, ordinal)"},
    {nullptr, nullptr, 0, nullptr},
};
PyType_Slot col_slots[] = {
    {Py_tp_dealloc, reinterpret_cast<void *>(col_dealloc)},
    {Py_tp_methods, col_methods},
    {Py_sq_length, reinterpret_cast<void *>(col_len)},
    {Py_bf_getbuffer, reinterpret_cast<void *>(col_getbuffer)},
    {Py_tp_doc, const_cast<char *>(
        "One int64 column of a MatchColumns, a MatchSpans, a PatternCounts, a RowScores or a RowOffsets, or one part of a FilteredRows, a MaskedRows or a MatchSnippets (int64; their data: uint8): len(), __dlpack__ / __dlpack_device__ (torch.from_dlpack, numpy.from_dlpack: no "
        "copy) and, in host memory, the buffer protocol (format 'q', or 'B' for uint8; read-only).")},
    {0, nullptr},
};

// ---------------------------------------------------------------------------
// The result types: MatchColumns, PatternCounts, FilteredRows, RowScores, MaskedRows, RowOffsets, MatchSpans, MatchSnippets.
// What tells one from another -- how long a part is, what tolist() gives, the attributes that are no parts -- and
// RESULT_TYPES, the one list of it.  The methods that make them follow.
// ---------------------------------------------------------------------------
// every part of every result type: `which` is the PyGetSetDef's closure
void *part(int which) { return reinterpret_cast<void *>(static_cast<intptr_t>(which)); }
PyObject *owner_get_part(PyObject *s, void *which) {
    int elem = 0;
    const uint64_t len = owner_of(s)->rt->part_len(owner_of(s), (int)reinterpret_cast<intptr_t>(which), &elem);
    if (len == NO_PART) Py_RETURN_NONE;
    return new_column(s, (int)reinterpret_cast<intptr_t>(which), len, elem);
}
// a size of the result as len(self) / as an attribute
template <typename T, uint64_t (*Size)(const T *)> Py_ssize_t size_len(PyObject *s) { return (Py_ssize_t)Size(handle<T>(s)); }
template <typename T, uint64_t (*Size)(const T *)> PyObject *size_get(PyObject *s, void *) { return PyLong_FromUnsignedLongLong(Size(handle<T>(s))); }

// tolist() of a result whose parts are int64 columns of n entries: the tuples (parts[0][i], parts[1][i], ..) as one list or,
// ro_part >= 0, as one list per row (rows + 1 row offsets).  The copies run with the GIL released.
template <typename T, int (*Copy)(const T *, int, int64_t *)>
PyObject *tuples_tolist(PyObject *self, const std::vector<int> &parts, uint64_t n, int ro_part, uint64_t rows) {
    const T *h = handle<T>(self);
    std::vector<std::vector<int64_t>> col(parts.size(), std::vector<int64_t>((size_t)n));
    std::vector<int64_t> ro(ro_part >= 0 ? (size_t)rows + 1 : 0);
    const int rc = nogil([&] {
        int rc = ACX_OK;
        for (size_t k = 0; k < parts.size() && rc == ACX_OK; k++) rc = Copy(h, parts[k], col[k].data());
        if (rc == ACX_OK && ro_part >= 0) rc = Copy(h, ro_part, ro.data());
        return rc;
    });
    if (rc != ACX_OK) return raise_acx(rc);
    return rows_of(ro_part >= 0 ? &ro : nullptr, n, [&](uint64_t i) {
        PyObject *t = PyTuple_New((Py_ssize_t)col.size());
        for (size_t k = 0; t && k < col.size(); k++) {
            PyObject *x = PyLong_FromUnsignedLongLong((unsigned long long)col[k][(size_t)i]);
            if (!x) { Py_CLEAR(t); break; }
            PyTuple_SET_ITEM(t, (Py_ssize_t)k, x);
        }
        return t;
    });
}

// MatchColumns: exactly what find_matches_as_indexes / _batch returns for the same arguments
uint64_t mc_part_len(const OwnerObject *o, int which, int *) {
    if (which != ACX_COL_ROW_OFFSETS) return acx_columns_count(handle<acx_columns_t>(o));
    return static_cast<const MatchColumnsObject *>(o)->batch ? acx_columns_rows(handle<acx_columns_t>(o)) + 1 : NO_PART;
}
PyObject *mc_tolist(PyObject *self, PyObject *) {
    const acx_columns_t *c = handle<acx_columns_t>(self);
    return tuples_tolist<acx_columns_t, acx_columns_copy>(self, {ACX_COL_PATTERN, ACX_COL_START, ACX_COL_END}, acx_columns_count(c),
                                                          static_cast<MatchColumnsObject *>(owner_of(self))->batch ? ACX_COL_ROW_OFFSETS : -1, acx_columns_rows(c));
}

// MatchSpans: list[tuple[int, int]], or one such list per row
uint64_t ms_part_len(const OwnerObject *o, int which, int *) {
    if (which != ACX_SPAN_ROW_OFFSETS) return acx_spans_count(handle<acx_spans_t>(o));
    return static_cast<const MatchSpansObject *>(o)->batch ? acx_spans_rows(handle<acx_spans_t>(o)) + 1 : NO_PART;
}
PyObject *ms_tolist(PyObject *self, PyObject *) {
    const acx_spans_t *c = handle<acx_spans_t>(self);
    return tuples_tolist<acx_spans_t, acx_spans_copy>(self, {ACX_SPAN_START, ACX_SPAN_END}, acx_spans_count(c),
                                                      static_cast<MatchSpansObject *>(owner_of(self))->batch ? ACX_SPAN_ROW_OFFSETS : -1, acx_spans_rows(c));
}

// PatternCounts: one list per haystack of (pattern, count), patterns ascending
uint64_t pc_part_len(const OwnerObject *o, int which, int *) {
    return which == ACX_TALLY_ROW_OFFSETS ? acx_tally_rows(handle<acx_tally_t>(o)) + 1 : acx_tally_nnz(handle<acx_tally_t>(o));
}
PyObject *pc_tolist(PyObject *self, PyObject *) {
    const acx_tally_t *t = handle<acx_tally_t>(self);
    return tuples_tolist<acx_tally_t, acx_tally_copy>(self, {ACX_TALLY_PATTERN, ACX_TALLY_COUNT}, acx_tally_nnz(t), ACX_TALLY_ROW_OFFSETS, acx_tally_rows(t));
}
PyObject *pc_get_shape(PyObject *s, void *) {
    return Py_BuildValue("(KK)", (unsigned long long)acx_tally_rows(handle<acx_tally_t>(s)),
                         (unsigned long long)static_cast<PatternCountsObject *>(owner_of(s))->n_patterns);
}

// FilteredRows: the kept rows, list[str] of the str class (UTF-8 decoded), list[bytes] of the bytes class
uint64_t fr_part_len(const OwnerObject *o, int which, int *elem) {
    *elem = which == ACX_FILT_DATA;
    return which == ACX_FILT_DATA ? acx_filtered_bytes(handle<acx_filtered_t>(o)) : acx_filtered_rows(handle<acx_filtered_t>(o)) + (which == ACX_FILT_OFFSETS);
}
PyObject *fr_tolist(PyObject *self, PyObject *) {
    const acx_filtered_t *f = handle<acx_filtered_t>(self);
    const uint64_t k = acx_filtered_rows(f);
    std::vector<int64_t> off((size_t)k + 1);
    std::vector<uint8_t> data((size_t)acx_filtered_bytes(f) + 1);
    const int rc = nogil([&] {
        const int rc = acx_filtered_copy(f, ACX_FILT_OFFSETS, off.data());
        return rc == ACX_OK ? acx_filtered_copy(f, ACX_FILT_DATA, data.data()) : rc;
    });
    if (rc != ACX_OK) return raise_acx(rc);
    const bool utf8 = static_cast<FilteredRowsObject *>(owner_of(self))->utf8;
    return list_of(0, k, [&](uint64_t i) { return cut_item(data, off, i, utf8); });
}
PyObject *fr_get_source_rows(PyObject *s, void *) {
    return PyLong_FromUnsignedLongLong(static_cast<FilteredRowsObject *>(owner_of(s))->n_src);
}

// MatchSnippets: list[str] of the str class (UTF-8 decoded), list[bytes] of the bytes class; a batch: one such list per row
uint64_t sn_part_len(const OwnerObject *o, int which, int *elem) {
    const acx_snippets_t *c = handle<acx_snippets_t>(o);
    *elem = which == ACX_SNIP_DATA;
    if (which == ACX_SNIP_DATA) return acx_snippets_nbytes(c);
    if (which != ACX_SNIP_ROW_OFFSETS) return acx_snippets_count(c) + (which == ACX_SNIP_OFFSETS);
    return static_cast<const MatchSnippetsObject *>(o)->batch ? acx_snippets_rows(c) + 1 : NO_PART;
}
PyObject *sn_tolist(PyObject *self, PyObject *) {
    const acx_snippets_t *c = handle<acx_snippets_t>(self);
    const MatchSnippetsObject *o = static_cast<MatchSnippetsObject *>(owner_of(self));
    const uint64_t n = acx_snippets_count(c);
    std::vector<int64_t> off((size_t)n + 1), ro(o->batch ? (size_t)acx_snippets_rows(c) + 1 : 0);
    std::vector<uint8_t> data((size_t)acx_snippets_nbytes(c) + 1);
    const int rc = nogil([&] {
        int rc = acx_snippets_copy(c, ACX_SNIP_OFFSETS, off.data());
        if (rc == ACX_OK) rc = acx_snippets_copy(c, ACX_SNIP_DATA, data.data());
        if (rc == ACX_OK && o->batch) rc = acx_snippets_copy(c, ACX_SNIP_ROW_OFFSETS, ro.data());
        return rc;
    });
    if (rc != ACX_OK) return raise_acx(rc);
    return rows_of(o->batch ? &ro : nullptr, n, [&](uint64_t i) { return cut_item(data, off, i, o->utf8); });
}

// MaskedRows: list[str] for mask_all_batch of the str class (a sequence of str: one entry per character), else list[bytes]
const void *masked_part(const acx_masked_t *m, int which) {
    return which == MR_OFFSETS ? static_cast<const void *>(acx_masked_offsets(m)) : acx_masked_data(m);
}
uint64_t mr_part_len(const OwnerObject *o, int which, int *elem) {
    *elem = which == MR_DATA;
    return which == MR_DATA ? acx_masked_bytes(handle<acx_masked_t>(o)) : acx_masked_rows(handle<acx_masked_t>(o)) + 1;
}
PyObject *mr_tolist(PyObject *self, PyObject *) {
    const acx_masked_t *m = handle<acx_masked_t>(self);
    const MaskedRowsObject *o = static_cast<MaskedRowsObject *>(owner_of(self));
    const uint64_t k = acx_masked_rows(m);
    std::vector<int64_t> off((size_t)k + 1);
    std::vector<uint8_t> data((size_t)acx_masked_bytes(m) + 1);
    const int rc = nogil([&] {
        const int rc = acx_masked_copy_offsets(m, off.data());
        return rc == ACX_OK ? acx_masked_copy(m, data.data()) : rc;
    });
    if (rc != ACX_OK) return raise_acx(rc);
    return list_of(0, k, [&](uint64_t i) {
        if (!o->src) return cut_item(data, off, i, o->utf8 && o->text);
        return per_character(o->src->data() + off[(size_t)i], data.data() + off[(size_t)i], (size_t)(off[(size_t)i + 1] - off[(size_t)i]), o->text);
    });
}
void mr_dealloc(PyObject *self) {
    delete static_cast<MaskedRowsObject *>(owner_of(self))->src;
    owner_dealloc(self);
}

// TokenLabels: list[tuple[int, int]] of (pattern, begin), or one such list per row for the sequence form
const void *labels_part(const acx_token_labels_t *l, int which) {
    return which == TL_PATTERN ? static_cast<const void *>(acx_token_labels_pattern(l)) : acx_token_labels_begin(l);
}
uint64_t tl_part_len(const OwnerObject *o, int which, int *elem) {
    *elem = which == TL_BEGIN;
    return acx_token_labels_count(handle<acx_token_labels_t>(o));
}
PyObject *tl_tolist(PyObject *self, PyObject *) {
    const acx_token_labels_t *l = handle<acx_token_labels_t>(self);
    const uint64_t n = acx_token_labels_count(l);
    std::vector<int64_t> pattern((size_t)n + 1);
    std::vector<uint8_t> begin((size_t)n + 1);
    const int rc = nogil([&] {
        const int rc = acx_token_labels_copy_pattern(l, pattern.data());
        return rc == ACX_OK ? acx_token_labels_copy_begin(l, begin.data()) : rc;
    });
    if (rc != ACX_OK) return raise_acx(rc);
    return rows_of(static_cast<TokenLabelsObject *>(owner_of(self))->row_offsets, n,
                   [&](uint64_t i) { return Py_BuildValue("(Li)", (long long)pattern[(size_t)i], (int)begin[(size_t)i]); });
}
PyObject *tl_get_row_offsets(PyObject *s, void *) {
    const std::vector<int64_t> *ro = static_cast<TokenLabelsObject *>(owner_of(s))->row_offsets;
    if (!ro) Py_RETURN_NONE;
    return list_of(0, ro->size(), [&](uint64_t i) { return PyLong_FromLongLong((long long)(*ro)[(size_t)i]); });
}
void tl_dealloc(PyObject *self) {
    TokenLabelsObject *o = static_cast<TokenLabelsObject *>(owner_of(self));
    delete o->row_offsets;
    PyObject *inputs[3] = {o->inputs[0], o->inputs[1], o->inputs[2]};
    owner_dealloc(self); // (waits for the stage: nothing reads the inputs after it)
    for (PyObject *cap : inputs) dlpack_release(cap);
}

// MatchesAt: list[tuple[int, int]] of (pattern, end) per anchor, or -- overlapping -- one such list per anchor
const void *at_part(const acx_at_t *r, int which) {
    return which == ACX_AT_PATTERN ? acx_at_pattern(r) : which == ACX_AT_END ? acx_at_end(r) : acx_at_row_offsets(r);
}
uint64_t at_part_len(const OwnerObject *o, int which, int *) {
    const acx_at_t *r = handle<acx_at_t>(o);
    if (which != ACX_AT_ROW_OFFSETS) return acx_at_entries(r);
    return acx_at_row_offsets(r) ? acx_at_count(r) + 1 : NO_PART;
}
PyObject *at_tolist(PyObject *self, PyObject *) {
    const acx_at_t *r = handle<acx_at_t>(self);
    const uint64_t n = acx_at_entries(r), anchors = acx_at_count(r);
    std::vector<int64_t> pattern((size_t)n + 1), end((size_t)n + 1), ro;
    bool csr = false;
    const int rc = nogil([&] {
        csr = acx_at_row_offsets(r) != nullptr; // (waits for the walk)
        if (csr) ro.assign((size_t)anchors + 1, 0);
        int rc = acx_at_copy(r, ACX_AT_PATTERN, pattern.data());
        if (rc == ACX_OK) rc = acx_at_copy(r, ACX_AT_END, end.data());
        if (rc == ACX_OK && csr) rc = acx_at_copy(r, ACX_AT_ROW_OFFSETS, ro.data());
        return rc;
    });
    if (rc != ACX_OK) return raise_acx(rc);
    return rows_of(csr ? &ro : nullptr, n,
                   [&](uint64_t i) { return Py_BuildValue("(LL)", (long long)pattern[(size_t)i], (long long)end[(size_t)i]); });
}
void at_dealloc(PyObject *self) {
    MatchesAtObject *o = static_cast<MatchesAtObject *>(owner_of(self));
    PyObject *inputs[3] = {o->inputs[0], o->inputs[1], o->inputs[2]};
    owner_dealloc(self); // (waits for the walk: nothing reads the inputs after it)
    for (PyObject *cap : inputs) dlpack_release(cap);
}

// Segments: list[tuple[int, int, int]] of (pattern, start, end) local to the row, or -- a batch -- one such list per row
const void *seg_part(const acx_seg_t *r, int which) {
    return which == ACX_SEG_PATTERN ? acx_seg_pattern(r) : which == ACX_SEG_OFFSETS ? acx_seg_offsets(r) : acx_seg_row_offsets(r);
}
uint64_t seg_part_len(const OwnerObject *o, int which, int *) {
    const acx_seg_t *r = handle<acx_seg_t>(o);
    if (which == ACX_SEG_PATTERN) return acx_seg_count(r);
    if (which == ACX_SEG_OFFSETS) return acx_seg_count(r) + 1;
    return static_cast<const SegmentsObject *>(o)->batch ? acx_seg_rows(r) + 1 : NO_PART;
}
PyObject *seg_tolist(PyObject *self, PyObject *) {
    const acx_seg_t *r = handle<acx_seg_t>(self);
    const uint64_t n = acx_seg_count(r), rows = acx_seg_rows(r);
    std::vector<int64_t> pattern((size_t)n + 1), off((size_t)n + 1), ro((size_t)rows + 1);
    const int rc = nogil([&] {
        int rc = acx_seg_copy(r, ACX_SEG_PATTERN, pattern.data());
        if (rc == ACX_OK) rc = acx_seg_copy(r, ACX_SEG_OFFSETS, off.data());
        if (rc == ACX_OK) rc = acx_seg_copy(r, ACX_SEG_ROW_OFFSETS, ro.data());
        return rc;
    });
    if (rc != ACX_OK) return raise_acx(rc);
    // (a row's first piece begins where the row does: the pieces tile it)
    uint64_t row = 0;
    return rows_of(static_cast<SegmentsObject *>(owner_of(self))->batch ? &ro : nullptr, n, [&](uint64_t i) {
        while (row + 1 < rows && (uint64_t)ro[(size_t)row + 1] <= i) row++;
        while (row > 0 && (uint64_t)ro[(size_t)row] > i) row--;
        const int64_t b = off[(size_t)ro[(size_t)row]];
        return Py_BuildValue("(LLL)", (long long)pattern[(size_t)i], (long long)(off[(size_t)i] - b), (long long)(off[(size_t)i + 1] - b));
    });
}
void seg_dealloc(PyObject *self) {
    SegmentsObject *o = static_cast<SegmentsObject *>(owner_of(self));
    PyObject *inputs[3] = {o->inputs[0], o->inputs[1], o->inputs[2]};
    owner_dealloc(self); // (waits for the kernels: nothing reads the inputs after it)
    for (PyObject *cap : inputs) dlpack_release(cap);
}

// WordPieces: list[tuple[int, int, int, int]] of (id, start, end, first) local to the row, or -- a batch -- one such list per row
const void *wp_part(const acx_wp_t *r, int which) {
    return which == ACX_WP_ID ? acx_wp_id(r) : which == ACX_WP_START ? acx_wp_start(r) : which == ACX_WP_END ? acx_wp_end(r)
           : which == ACX_WP_FIRST ? (const void *)acx_wp_first(r) : acx_wp_row_offsets(r);
}
uint64_t wp_part_len(const OwnerObject *o, int which, int *elem) {
    const acx_wp_t *r = handle<acx_wp_t>(o);
    *elem = which == ACX_WP_FIRST;
    if (which != ACX_WP_ROW_OFFSETS) return acx_wp_count(r);
    return static_cast<const WordPiecesObject *>(o)->batch ? acx_wp_rows(r) + 1 : NO_PART;
}
PyObject *wp_tolist(PyObject *self, PyObject *) {
    const acx_wp_t *r = handle<acx_wp_t>(self);
    const WordPiecesObject *o = static_cast<WordPiecesObject *>(owner_of(self));
    const uint64_t n = acx_wp_count(r), rows = acx_wp_rows(r);
    std::vector<int64_t> id((size_t)n + 1), start((size_t)n + 1), end((size_t)n + 1), ro((size_t)rows + 1), begin((size_t)rows + 1, 0);
    std::vector<uint8_t> first((size_t)n + 1);
    const int rc = nogil([&] {
        int rc = acx_wp_copy(r, ACX_WP_ID, id.data());
        if (rc == ACX_OK) rc = acx_wp_copy(r, ACX_WP_START, start.data());
        if (rc == ACX_OK) rc = acx_wp_copy(r, ACX_WP_END, end.data());
        if (rc == ACX_OK) rc = acx_wp_copy(r, ACX_WP_FIRST, first.data());
        if (rc == ACX_OK) rc = acx_wp_copy(r, ACX_WP_ROW_OFFSETS, ro.data());
        if (rc == ACX_OK && o->batch && !o->row_begin && !o->row_length && o->d_off)
            rc = acx_device_download(begin.data(), o->d_off, (rows + 1) * 8);
        return rc;
    });
    if (rc != ACX_OK) return raise_acx(rc);
    if (o->batch && o->row_begin) begin = *o->row_begin;
    else if (o->batch && o->row_length)
        for (uint64_t h = 0; h <= rows; h++) begin[(size_t)h] = (int64_t)(h * o->row_length);
    uint64_t row = 0;
    return rows_of(o->batch ? &ro : nullptr, n, [&](uint64_t i) {
        while (row + 1 < rows && (uint64_t)ro[(size_t)row + 1] <= i) row++;
        while (row > 0 && (uint64_t)ro[(size_t)row] > i) row--;
        const int64_t b = begin[(size_t)row];
        return Py_BuildValue("(LLLi)", (long long)id[(size_t)i], (long long)(start[(size_t)i] - b), (long long)(end[(size_t)i] - b),
                             (int)first[(size_t)i]);
    });
}
void wp_dealloc(PyObject *self) {
    WordPiecesObject *o = static_cast<WordPiecesObject *>(owner_of(self));
    delete o->row_begin;
    PyObject *inputs[3] = {o->inputs[0], o->inputs[1], o->inputs[2]};
    owner_dealloc(self); // (waits for the kernels: nothing reads the inputs after it)
    for (PyObject *cap : inputs) dlpack_release(cap);
}

// RowScores and RowOffsets: their one part as list[int]
uint64_t rs_part_len(const OwnerObject *o, int, int *) { return acx_scores_rows(handle<acx_scores_t>(o)); }
uint64_t ro_part_len(const OwnerObject *o, int, int *) { return acx_rows_count(handle<acx_rows_t>(o)) + 1; }
template <typename T, int (*Copy)(const T *, int64_t *)> PyObject *words_tolist(PyObject *self, PyObject *) {
    int elem = 0;
    const uint64_t n = owner_of(self)->rt->part_len(owner_of(self), 0, &elem);
    std::vector<int64_t> v((size_t)n + 1);
    const int rc = nogil([&] { return Copy(handle<T>(self), v.data()); });
    if (rc != ACX_OK) return raise_acx(rc);
    return list_of(0, n, [&](uint64_t i) { return PyLong_FromLongLong((long long)v[(size_t)i]); });
}

#define DEVICE_ATTR(what) {"device", owner_get_device, nullptr, "None: the " what " in host memory; otherwise the HIP ordinal they lie on", nullptr}
ResultType RESULT_TYPES[RT_COUNT] = {
    {"ahocorasick_rs.MatchColumns", sizeof(MatchColumnsObject), owner_ops<acx_columns_t, acx_columns_on_device, acx_columns_data, acx_free_columns>(),
     mc_part_len, size_len<acx_columns_t, acx_columns_count>, mc_tolist,
     "what find_matches_as_indexes / find_matches_as_indexes_batch returns for the same arguments (copies device columns "
     "to the host)",
     "The matches of find_matches_as_columns / _batch: .pattern, .start, .end (and .row_offsets for a batch) are Column "
     "objects of len(self) int64 entries, where the search ran (.device).  Every accessor of a column waits for the "
     "split kernel first.",
     {{"pattern", owner_get_part, nullptr, "Column: the pattern index of every match", part(ACX_COL_PATTERN)},
      {"start", owner_get_part, nullptr, "Column: where every match starts", part(ACX_COL_START)},
      {"end", owner_get_part, nullptr, "Column: where every match ends", part(ACX_COL_END)},
      {"row_offsets", owner_get_part, nullptr,
       "None for one haystack; for a batch a Column of len(haystacks) + 1 entries: rows row_offsets[h] .. row_offsets[h + 1] "
       "are haystack h's matches", part(ACX_COL_ROW_OFFSETS)},
      DEVICE_ATTR("columns are")}},
    {"ahocorasick_rs.PatternCounts", sizeof(PatternCountsObject), owner_ops<acx_tally_t, acx_tally_on_device, acx_tally_data, acx_free_tally>(),
     pc_part_len, size_len<acx_tally_t, acx_tally_nnz>, pc_tolist,
     "one list per haystack of (pattern, count) tuples, patterns ascending (copies device parts to the host)",
     "The result of count_by_pattern_sparse_batch: the CSR form of the haystacks x patterns matrix of match counts.  "
     ".row_offsets, .pattern and .count are Column objects (int64) where the search ran (.device); len(self) is the "
     "number of non-zero entries.  torch.sparse_csr_tensor(*map(torch.from_dlpack, (pc.row_offsets, pc.pattern, pc.count)), "
     "size=pc.shape) is the matrix, without a copy.",
     {{"row_offsets", owner_get_part, nullptr,
       "Column of shape[0] + 1 entries from 0: entries row_offsets[h] .. row_offsets[h + 1] of pattern and count are haystack h's",
       part(ACX_TALLY_ROW_OFFSETS)},
      {"pattern", owner_get_part, nullptr, "Column of len(self) pattern indexes, strictly ascending within a row", part(ACX_TALLY_PATTERN)},
      {"count", owner_get_part, nullptr, "Column of len(self) counts, all >= 1", part(ACX_TALLY_COUNT)},
      {"shape", pc_get_shape, nullptr, "(haystacks, patterns): the size of the matrix", nullptr},
      DEVICE_ATTR("parts are")}},
    {"ahocorasick_rs.FilteredRows", sizeof(FilteredRowsObject), owner_ops<acx_filtered_t, acx_filtered_on_device, acx_filtered_data, acx_free_filtered>(),
     fr_part_len, size_len<acx_filtered_t, acx_filtered_rows>, fr_tolist,
     "the kept rows as list[str] (the str class: UTF-8 decoded) or list[bytes] (copies device parts to the host)",
     "The result of filter_batch: the kept rows of a batch as a compacted batch.  .rows and .offsets are int64 Column "
     "objects, .data a uint8 one, where the search ran (.device); len(self) is the number of kept rows, .nbytes the size "
     "of .data, .source_rows the rows of the batch.  Kept row i is source row rows[i] = data[offsets[i]:offsets[i + 1]].",
     {{"rows", owner_get_part, nullptr, "Column of len(self) int64 entries: the kept source row indexes, strictly ascending", part(ACX_FILT_ROWS)},
      {"offsets", owner_get_part, nullptr, "Column of len(self) + 1 int64 entries from 0: kept row i is data[offsets[i]:offsets[i + 1]]",
       part(ACX_FILT_OFFSETS)},
      {"data", owner_get_part, nullptr, "Column of nbytes uint8 entries: the kept rows' own bytes back to back", part(ACX_FILT_DATA)},
      DEVICE_ATTR("parts are"),
      {"nbytes", size_get<acx_filtered_t, acx_filtered_bytes>, nullptr, "the size of data", nullptr},
      {"source_rows", fr_get_source_rows, nullptr, "the rows of the batch that was filtered", nullptr}}},
    {"ahocorasick_rs.RowScores", sizeof(OwnerObject), owner_ops<acx_scores_t, acx_scores_on_device, acx_scores_data, acx_free_scores>(),
     rs_part_len, size_len<acx_scores_t, acx_scores_rows>, words_tolist<acx_scores_t, acx_scores_copy>,
     "the scores as list[int] (copies device scores to the host)",
     "The result of score_batch: .score is an int64 Column of len(self) entries, one per row of the batch, where the "
     "search ran (.device).",
     {{"score", owner_get_part, nullptr, "Column of len(self) int64 entries: every row's score", nullptr},
      DEVICE_ATTR("scores are")}},
    {"ahocorasick_rs.MaskedRows", sizeof(MaskedRowsObject), owner_ops<acx_masked_t, acx_masked_on_device, masked_part, acx_free_masked>(),
     mr_part_len, size_len<acx_masked_t, acx_masked_rows>, mr_tolist,
     "the rows as list[str] (mask_all_batch of the str class) or list[bytes] (copies device parts to the host); for a sequence "
     "of str one entry per character",
     "The result of mask_all_batch / match_mask_batch: .data is a uint8 Column of nbytes entries in the input's own layout "
     "-- fill (or 1) where a match covers a byte -- and .offsets an int64 Column of len(self) + 1 entries from 0, where the "
     "search ran (.device); len(self) is the number of rows.  For a tensor input the caller's own offsets cut .data as well.",
     {{"data", owner_get_part, nullptr, "Column of nbytes uint8 entries: the rows back to back, in the input's own layout", part(MR_DATA)},
      {"offsets", owner_get_part, nullptr, "Column of len(self) + 1 int64 entries from 0: row i is data[offsets[i]:offsets[i + 1]]", part(MR_OFFSETS)},
      DEVICE_ATTR("parts are"),
      {"nbytes", size_get<acx_masked_t, acx_masked_bytes>, nullptr, "the size of data: the input's", nullptr}},
     mr_dealloc},
    {"ahocorasick_rs.RowOffsets", sizeof(OwnerObject), owner_ops<acx_rows_t, acx_rows_on_device, acx_rows_offsets, acx_free_rows>(),
     ro_part_len, size_len<acx_rows_t, acx_rows_count>, words_tolist<acx_rows_t, acx_rows_copy>,
     "the offsets as list[int] (copies device offsets to the host)",
     "The result of split_rows: .offsets is an int64 Column of len(self) + 1 entries that rise strictly from 0 to .nbytes, "
     "where the data lies (.device); len(self) is the number of rows.  Pass .offsets as offsets= to the _batch methods.",
     {{"offsets", owner_get_part, nullptr, "Column of len(self) + 1 int64 entries from 0 to nbytes: row i is data[offsets[i]:offsets[i + 1]]", nullptr},
      DEVICE_ATTR("offsets are"),
      {"nbytes", size_get<acx_rows_t, acx_rows_bytes>, nullptr, "the length of the data that was cut", nullptr}}},
    {"ahocorasick_rs.MatchSpans", sizeof(MatchSpansObject), owner_ops<acx_spans_t, acx_spans_on_device, acx_spans_data, acx_free_spans>(),
     ms_part_len, size_len<acx_spans_t, acx_spans_count>, ms_tolist,
     "the spans as list[tuple[int, int]] of (start, end), or one such list per row of a batch (copies device columns to the "
     "host)",
     "The merged spans of cover_spans / cover_spans_batch: .start and .end (and .row_offsets for a batch) are Column "
     "objects of len(self) int64 entries, where the search ran (.device).  Every accessor of a column waits for the "
     "stage's last kernel first.",
     {{"start", owner_get_part, nullptr, "Column: where every span starts", part(ACX_SPAN_START)},
      {"end", owner_get_part, nullptr, "Column: where every span ends", part(ACX_SPAN_END)},
      {"row_offsets", owner_get_part, nullptr,
       "None for one haystack; for a batch a Column of len(haystacks) + 1 entries: spans row_offsets[h] .. row_offsets[h + 1] "
       "are haystack h's", part(ACX_SPAN_ROW_OFFSETS)},
      DEVICE_ATTR("columns are")}},
    {"ahocorasick_rs.MatchSnippets", sizeof(MatchSnippetsObject), owner_ops<acx_snippets_t, acx_snippets_on_device, acx_snippets_data, acx_free_snippets>(),
     sn_part_len, size_len<acx_snippets_t, acx_snippets_count>, sn_tolist,
     "the snippets as list[str] (the str class: UTF-8 decoded) or list[bytes], or one such list per row of a batch (copies "
     "device parts to the host)",
     "The result of find_matches_as_snippets / find_matches_as_snippets_batch: one snippet per match.  .data is a uint8 "
     "Column of nbytes entries, .offsets, .pattern and .lead (and .row_offsets for a batch) are int64 Column objects, where "
     "the search ran (.device); len(self) is the number of snippets.  Every accessor of a part waits for the stage's last "
     "kernel first.",
     {{"data", owner_get_part, nullptr, "Column of nbytes uint8 entries: the snippets back to back", part(ACX_SNIP_DATA)},
      {"offsets", owner_get_part, nullptr, "Column of len(self) + 1 int64 entries from 0: snippet i is data[offsets[i]:offsets[i + 1]]",
       part(ACX_SNIP_OFFSETS)},
      {"pattern", owner_get_part, nullptr, "Column of len(self) int64 entries: the pattern of every match", part(ACX_SNIP_PATTERN)},
      {"lead", owner_get_part, nullptr,
       "Column of len(self) int64 entries: the bytes of snippet i that stand before the match, which begins at "
       "data[offsets[i] + lead[i]]", part(ACX_SNIP_LEAD)},
      {"row_offsets", owner_get_part, nullptr,
       "None for one haystack; for a batch a Column of len(haystacks) + 1 entries: snippets row_offsets[h] .. row_offsets[h + 1] "
       "are haystack h's", part(ACX_SNIP_ROW_OFFSETS)},
      DEVICE_ATTR("parts are"),
      {"nbytes", size_get<acx_snippets_t, acx_snippets_nbytes>, nullptr, "the size of data", nullptr}}},
    {"ahocorasick_rs.TokenLabels", sizeof(TokenLabelsObject), owner_ops<acx_token_labels_t, acx_token_labels_on_device, labels_part, acx_free_token_labels>(),
     tl_part_len, size_len<acx_token_labels_t, acx_token_labels_count>, tl_tolist,
     "the labels as list[tuple[int, int]] of (pattern, begin), or one such list per row for a sequence of haystacks (copies "
     "device columns to the host)",
     "The result of label_tokens / label_tokens_batch: one entry per token.  .pattern is an int64 Column -- the pattern of the "
     "first match (in the search's order) that touches the token, or -1 -- and .begin a uint8 Column -- 1 where a match's "
     "tokens begin, the B of BIO -- where the search ran (.device); len(self) is the number of tokens.  pattern >= 0 is the "
     "token mask.  Every accessor of a column waits for the stage's last kernel first.",
     {{"pattern", owner_get_part, nullptr, "Column of len(self) int64 entries: the owner's pattern, or -1", part(TL_PATTERN)},
      {"begin", owner_get_part, nullptr, "Column of len(self) uint8 entries: 1 iff the token is the first of its owner's", part(TL_BEGIN)},
      {"row_offsets", tl_get_row_offsets, nullptr,
       "None for one haystack and for a tensor; for a sequence of haystacks a list of len(haystacks) + 1 ints: tokens "
       "row_offsets[h] .. row_offsets[h + 1] - 1 are haystack h's", nullptr},
      DEVICE_ATTR("columns are")},
     tl_dealloc},
    {"ahocorasick_rs.MatchesAt", sizeof(MatchesAtObject), owner_ops<acx_at_t, acx_at_on_device, at_part, acx_free_at>(),
     at_part_len, size_len<acx_at_t, acx_at_count>, at_tolist,
     "the result as list[tuple[int, int]] of (pattern, end), one per anchor, or -- overlapping -- one such list per anchor "
     "(copies device columns to the host)",
     "The result of match_at / match_prefix_batch: which pattern begins exactly at every anchor -- a position, or the start of "
     "a row.  .pattern and .end are int64 Columns where the walk ran (.device): one entry per anchor, (-1, -1) where no pattern "
     "begins; overlapping: every such pattern, ordered by end, then by pattern, and .row_offsets cuts the entries by anchor.  "
     "len(self) is the number of anchors.  Every accessor of a column waits for the walk's last kernel first.",
     {{"pattern", owner_get_part, nullptr, "Column of int64 entries: the pattern that begins at the anchor, or -1", part(ACX_AT_PATTERN)},
      {"end", owner_get_part, nullptr, "Column of int64 entries: where that pattern ends (match_prefix_batch: its length), or -1", part(ACX_AT_END)},
      {"row_offsets", owner_get_part, nullptr,
       "None unless overlapping; else a Column of len(self) + 1 int64 entries: entries row_offsets[k] .. row_offsets[k + 1] - 1 "
       "are anchor k's", part(ACX_AT_ROW_OFFSETS)},
      DEVICE_ATTR("columns are")},
     at_dealloc},
    {"ahocorasick_rs.Segments", sizeof(SegmentsObject), owner_ops<acx_seg_t, acx_seg_on_device, seg_part, acx_free_seg>(),
     seg_part_len, size_len<acx_seg_t, acx_seg_count>, seg_tolist,
     "the pieces as list[tuple[int, int, int]] of (pattern, start, end) local to their row, or -- segment_batch -- one such "
     "list per row (copies device columns to the host)",
     "The result of segment / segment_batch: the data cut into dictionary entries from left to right.  .pattern is an int64 "
     "Column of len(self) entries -- the pattern of every piece, or -1 for an unknown unit -- and .offsets an int64 Column of "
     "len(self) + 1 GLOBAL ascending boundaries that ends at the data's length: what label_tokens_batch takes as "
     "token_offsets.  .row_offsets (segment_batch) cuts the pieces by row.  All lie where the chain ran (.device).  Every "
     "accessor of a column waits for the stage's last kernel first.",
     {{"pattern", owner_get_part, nullptr, "Column of len(self) int64 entries: the pattern of the piece, or -1", part(ACX_SEG_PATTERN)},
      {"offsets", owner_get_part, nullptr,
       "Column of len(self) + 1 int64 entries: piece i is data[offsets[i]:offsets[i + 1]] (characters for a str)", part(ACX_SEG_OFFSETS)},
      {"row_offsets", owner_get_part, nullptr,
       "None for one haystack; for a batch a Column of len(haystacks) + 1 int64 entries: pieces row_offsets[h] .. "
       "row_offsets[h + 1] - 1 are haystack h's", part(ACX_SEG_ROW_OFFSETS)},
      DEVICE_ATTR("columns are")},
     seg_dealloc},
    {"ahocorasick_rs.WordPieces", sizeof(WordPiecesObject), owner_ops<acx_wp_t, acx_wp_on_device, wp_part, acx_free_wp>(),
     wp_part_len, size_len<acx_wp_t, acx_wp_count>, wp_tolist,
     "the pieces as list[tuple[int, int, int, int]] of (id, start, end, first) local to their row, or -- wordpiece_batch -- one "
     "such list per row (copies device columns to the host)",
     "The result of wordpiece / wordpiece_batch: the words of the data cut into vocabulary entries.  .id, .start and .end are "
     "int64 Columns of len(self) entries -- the pattern of every piece, or unk_id, and its GLOBAL positions -- and .first a "
     "uint8 Column: 1 on the first piece of its word.  .row_offsets (wordpiece_batch) cuts the pieces by row.  All lie where "
     "the chains ran (.device).  Every accessor of a column waits for the stage's last kernel first.",
     {{"id", owner_get_part, nullptr, "Column of len(self) int64 entries: the pattern of the piece, or unk_id", part(ACX_WP_ID)},
      {"start", owner_get_part, nullptr, "Column of len(self) int64 entries: where the piece begins (characters for a str)", part(ACX_WP_START)},
      {"end", owner_get_part, nullptr, "Column of len(self) int64 entries: where the piece ends (characters for a str)", part(ACX_WP_END)},
      {"first", owner_get_part, nullptr, "Column of len(self) uint8 entries: 1 iff the piece is the first of its word", part(ACX_WP_FIRST)},
      {"row_offsets", owner_get_part, nullptr,
       "None for one haystack; for a batch a Column of len(haystacks) + 1 int64 entries: pieces row_offsets[h] .. "
       "row_offsets[h + 1] - 1 are haystack h's", part(ACX_WP_ROW_OFFSETS)},
      DEVICE_ATTR("columns are")},
     wp_dealloc},
};
#undef DEVICE_ATTR

// one result type of the table as a Python type in the module; false with the exception set
bool register_result_type(PyObject *module, ResultType *t) {
    t->getset.push_back({nullptr, nullptr, nullptr, nullptr, nullptr});
    t->methods[0] = {"tolist", t->tolist, METH_NOARGS, t->tolist_doc};
    t->methods[1] = {nullptr, nullptr, 0, nullptr};
    PyType_Slot slots[] = {
        {Py_tp_dealloc, reinterpret_cast<void *>(t->dealloc ? t->dealloc : owner_dealloc)},
        {Py_tp_methods, t->methods},
        {Py_tp_getset, t->getset.data()},
        {Py_sq_length, reinterpret_cast<void *>(t->len)},
        {Py_tp_doc, const_cast<char *>(t->doc)},
        {0, nullptr},
    };
    PyType_Spec spec = {t->name, t->size, 0, Py_TPFLAGS_DEFAULT | Py_TPFLAGS_DISALLOW_INSTANTIATION, slots};
    t->type = reinterpret_cast<PyTypeObject *>(PyType_FromSpec(&spec));
    if (!t->type) return false;
    Py_INCREF(t->type); // (the module holds one reference, the table the other)
    return PyModule_AddObject(module, strchr(t->name, '.') + 1, reinterpret_cast<PyObject *>(t->type)) == 0;
}

// find_matches_as_columns / _batch (code-point offsets when the str class's text is not ASCII).  The haystack arguments and
// their errors are find_matches_as_indexes' / _batch's.
template <bool batch> PyObject *columns(PyObject *self, PyObject *args, PyObject *kwargs) {
    acx_automaton_t *a = ac_of(self);
    const bool utf8 = utf8_of(self);
    const char *kw[] = {batch ? "haystacks" : "haystack", "overlapping", nullptr};
    PyObject *hay = nullptr, *ov = nullptr;
    int overlapping = 0;
    if (!PyArg_ParseTupleAndKeywords(args, kwargs, batch ? "O|O:find_matches_as_columns_batch" : "O|O:find_matches_as_columns",
                                     const_cast<char **>(kw), &hay, &ov))
        return nullptr;
    if (ov && !parse_bool(ov, "overlapping", &overlapping)) return nullptr;
    const int device = acx_automaton_device(a);
    acx_columns_t *c = nullptr;
    int rc;
    if (batch) {
        Packed in;
        if (!pack_sequence(hay, utf8, false, &in)) return nullptr;
        rc = nogil([&] {
            return acx_find_columns(a, in.blob.data(), in.off[(size_t)in.n], in.off.data(), (uint64_t)in.n, overlapping, utf8 && !in.all_ascii, &c);
        });
    } else {
        HaystackView v;
        if (!haystack_view(hay, utf8, true, device, &v)) return nullptr;
        rc = single_dispatch(
            device, v,
            [&](const uint8_t *p, uint64_t len) { return acx_find_columns(a, p, len, nullptr, 0, overlapping, utf8 && !v.is_ascii, &c); },
            [&](const uint8_t *p, uint64_t len) { return acx_find_columns_device(a, p, len, nullptr, 0, 0, overlapping, 0, &c); }); // (split where it lies)
    }
    if (rc != ACX_OK) return raise_acx(rc);
    OwnerObject *o = new_owner(RT_MATCH_COLUMNS, c, device);
    if (o) static_cast<MatchColumnsObject *>(o)->batch = batch;
    return reinterpret_cast<PyObject *>(o);
}

// ---------------------------------------------------------------------------
// per-haystack pattern counts: count_by_pattern_sparse_batch -> PatternCounts (acx_tally / acx_tally_device).  A
// PatternCounts owns the acx_tally_t; its three parts are Columns with the lifetime chain of a MatchColumns' columns.
// ---------------------------------------------------------------------------
// The haystacks of a _batch method: a sequence of str (utf8) / buffers packed into one blob with its offsets, or one 1-D
// uint8 __dlpack__ tensor that holds the rows back to back, cut by `offsets` (a 1-D int64 __dlpack__ tensor on the same
// device) or by `row_length`.  Kept in one place so that the other _batch methods can take it.
struct BatchInput {
    Packed seq; // a sequence
    // a tensor: `len` bytes at `p`, `rows` rows; d_off (its device's offsets) or row_length
    bool tensor = false, on_device = false;
    const uint8_t *p = nullptr;
    uint64_t len = 0, rows = 0, row_length = 0;
    const uint64_t *t_off = nullptr;
    PyObject *cap = nullptr, *cap_off = nullptr;
    BatchInput() = default;
    BatchInput(const BatchInput &) = delete;
    BatchInput &operator=(const BatchInput &) = delete;
    ~BatchInput() { dlpack_release(cap); dlpack_release(cap_off); }
};

// The tensor argument `name` that goes with a haystack tensor (offsets=, token_offsets): a 1-D contiguous int64 __dlpack__
// tensor where the haystack tensor lies (on_device: in HBM on want_device, else in host memory).  *cap: its capsule, the
// caller's to release (set as soon as it exists); *words / *entries: what it holds.  Sets the exception.
bool int64_tensor(PyObject *o, const char *name, bool on_device, int want_device, PyObject **cap, const uint64_t **words, uint64_t *entries) {
    if (!PyObject_HasAttrString(o, "__dlpack__")) {
        PyErr_Format(PyExc_TypeError, "argument '%s': '%.100s' object has no __dlpack__", name, Py_TYPE(o)->tp_name);
        return false;
    }
    *cap = PyObject_CallMethod(o, "__dlpack__", nullptr);
    if (!*cap) return false;
    DLManagedTensorC *mt = PyCapsule_IsValid(*cap, "dltensor")
                               ? static_cast<DLManagedTensorC *>(PyCapsule_GetPointer(*cap, "dltensor")) : nullptr;
    if (!mt) {
        PyErr_SetString(PyExc_TypeError, "__dlpack__ did not return a 'dltensor' capsule");
        return false;
    }
    const DLTensorC &t = mt->dl_tensor;
    if (t.ndim != 1 || t.dtype.code != 0 || t.dtype.bits != 64 || t.dtype.lanes != 1 ||
        (t.strides && t.shape[0] > 1 && t.strides[0] != 1)) {
        PyErr_Format(PyExc_TypeError, "%s must be a 1-D contiguous int64 tensor", name);
        return false;
    }
    const bool dev = t.device.device_type == kDLROCM || t.device.device_type == kDLCUDA;
    const bool host = t.device.device_type == kDLCPU || t.device.device_type == kDLROCMHost || t.device.device_type == kDLCUDAHost;
    if ((!dev && !host) || dev != on_device || (dev && t.device.device_id != want_device)) {
        PyErr_Format(PyExc_ValueError, "the %s tensor lies on another device than the haystack tensor", name);
        return false;
    }
    *words = reinterpret_cast<const uint64_t *>(static_cast<const uint8_t *>(t.data) + t.byte_offset);
    *entries = (uint64_t)t.shape[0];
    return true;
}

bool batch_input(PyObject *hay, PyObject *offsets, PyObject *row_length, bool utf8, int want_device, BatchInput *in) {
    if (offsets == Py_None) offsets = nullptr;
    if (row_length == Py_None) row_length = nullptr;
    const bool has_dlpack = !PyUnicode_Check(hay) && PyObject_HasAttrString(hay, "__dlpack__");
    in->tensor = has_dlpack && (!PyObject_CheckBuffer(hay) || offsets || row_length);
    if (!in->tensor) {
        if (offsets || row_length) {
            PyErr_SetString(PyExc_TypeError, "offsets / row_length cut ONE __dlpack__ tensor into rows: a sequence of haystacks takes neither");
            return false;
        }
        if (!pack_sequence(hay, utf8, false, &in->seq)) return false;
        in->rows = (uint64_t)in->seq.n;
        return true;
    }
    if ((offsets != nullptr) == (row_length != nullptr)) {
        PyErr_SetString(PyExc_TypeError, "a tensor of haystacks needs exactly one of offsets and row_length");
        return false;
    }
    in->cap = dlpack_view(hay, want_device, &in->p, &in->len, &in->on_device);
    if (!in->cap) return false;
    if (capsule_tensor(in->cap).ndim != 1) {
        PyErr_SetString(PyExc_TypeError, "Only one-dimensional sequences are supported");
        return false;
    }
    if (row_length) {
        long long rl;
        if (!parse_int(row_length, "row_length", &rl)) return false;
        if (rl <= 0 || in->len % (uint64_t)rl) {
            PyErr_SetString(PyExc_ValueError, "row_length must be positive and divide the tensor's length");
            return false;
        }
        in->row_length = (uint64_t)rl;
        in->rows = in->len / (uint64_t)rl;
        return true;
    }
    uint64_t entries = 0;
    if (!int64_tensor(offsets, "offsets", in->on_device, want_device, &in->cap_off, &in->t_off, &entries)) return false;
    if (entries < 1) {
        PyErr_SetString(PyExc_ValueError, "offsets needs rows + 1 entries: at least one");
        return false;
    }
    in->rows = entries - 1;
    if (!in->on_device) { // (device offsets: their ends are checked behind the producer's kernels, by the caller)
        const int64_t *o = reinterpret_cast<const int64_t *>(in->t_off);
        bool ok = o[0] == 0 && (uint64_t)o[in->rows] == in->len;
        for (uint64_t i = 0; ok && i < in->rows; i++) ok = o[i] <= o[i + 1];
        if (!ok) {
            PyErr_SetString(PyExc_ValueError, "offsets must rise from 0 to the tensor's length");
            return false;
        }
    }
    return true;
}

// One call on a BatchInput with the GIL released: host(p, len, offsets, rows) on a sequence or a host tensor,
// device(p, len, d_offsets, rows, row_length) on a tensor in HBM, behind the producer's kernels and the check of where its
// offsets begin and end (between the two they are the caller's word).  Returns the call's status; BAD_OFFSETS with the
// ValueError set for offsets that do not span the tensor.
constexpr int BAD_OFFSETS = -1000;
template <typename Host, typename Device>
int batch_dispatch(int device_ordinal, const BatchInput &in, Host &&host, Device &&device) {
    int rc;
    bool bad_offsets = false;
    std::vector<uint64_t> cut;
    if (in.tensor && !in.on_device && in.row_length) {
        cut.resize((size_t)in.rows + 1);
        for (uint64_t i = 0; i <= in.rows; i++) cut[(size_t)i] = i * in.row_length;
    }
    Py_BEGIN_ALLOW_THREADS
    if (!in.tensor) {
        rc = host(in.seq.blob.data(), in.seq.off[(size_t)in.rows], in.seq.off.data(), in.rows);
    } else if (!in.on_device) {
        rc = host(in.p, in.len, in.row_length ? cut.data() : in.t_off, in.rows);
    } else {
        rc = acx_device_synchronize_on(device_ordinal); // (the producer's kernels may still write the tensors)
        if (rc == ACX_OK && in.t_off) {
            uint64_t ends[2] = {1, 0};
            rc = acx_device_download(&ends[0], in.t_off, 8);
            if (rc == ACX_OK) rc = acx_device_download(&ends[1], in.t_off + in.rows, 8);
            bad_offsets = rc == ACX_OK && (ends[0] != 0 || ends[1] != in.len);
        }
        if (rc == ACX_OK && !bad_offsets) rc = device(in.p, in.len, in.t_off, in.rows, in.row_length);
    }
    Py_END_ALLOW_THREADS
    if (!bad_offsets) return rc;
    PyErr_SetString(PyExc_ValueError, "offsets must rise from 0 to the tensor's length");
    return BAD_OFFSETS;
}

// count_by_pattern_sparse_batch (no offset is reported: the str class's search is on bytes too)
PyObject *sparse_counts(PyObject *self, PyObject *args, PyObject *kwargs) {
    acx_automaton_t *a = ac_of(self);
    const bool utf8 = utf8_of(self);
    static const char *kw[] = {"haystacks", "overlapping", "offsets", "row_length", nullptr};
    PyObject *hay = nullptr, *ov = nullptr, *offsets = nullptr, *row_length = nullptr;
    int overlapping = 0;
    if (!PyArg_ParseTupleAndKeywords(args, kwargs, "O|O$OO:count_by_pattern_sparse_batch", const_cast<char **>(kw), &hay, &ov,
                                     &offsets, &row_length))
        return nullptr;
    if (ov && !parse_bool(ov, "overlapping", &overlapping)) return nullptr;
    const int device = acx_automaton_device(a);
    BatchInput in;
    if (!batch_input(hay, offsets, row_length, utf8, device, &in)) return nullptr;
    acx_info_t info;
    if (acx_automaton_info(a, &info) != ACX_OK) return raise_acx(ACX_EINVAL);
    acx_tally_t *t = nullptr;
    const int rc = batch_dispatch(
        device, in,
        [&](const uint8_t *p, uint64_t len, const uint64_t *off, uint64_t rows) { return acx_tally(a, p, len, off, rows, overlapping, &t); },
        [&](const uint8_t *p, uint64_t len, const uint64_t *d_off, uint64_t rows, uint64_t row_length) {
            return acx_tally_device(a, p, len, d_off, rows, row_length, overlapping, &t);
        });
    if (rc == BAD_OFFSETS) return nullptr;
    if (rc != ACX_OK) return raise_acx(rc);
    OwnerObject *o = new_owner(RT_PATTERN_COUNTS, t, device);
    if (o) static_cast<PatternCountsObject *>(o)->n_patterns = info.n_patterns;
    return reinterpret_cast<PyObject *>(o);
}

// ---------------------------------------------------------------------------
// rows kept or dropped by match: filter_batch -> FilteredRows (acx_filter / acx_filter_device).  A FilteredRows owns the
// acx_filtered_t; its three parts are Columns (rows and offsets int64, data uint8) with the lifetime chain of a
// MatchColumns' columns.
// ---------------------------------------------------------------------------
// keep = 'unmatched' | 'matched' -> the acx_filter* flags; sets the exception
bool parse_keep(PyObject *keep, uint32_t *flags) {
    if (!PyUnicode_Check(keep)) {
        PyErr_Format(PyExc_TypeError, "argument 'keep': '%.100s' object cannot be converted to 'PyString'", Py_TYPE(keep)->tp_name);
        return false;
    }
    if (PyUnicode_CompareWithASCIIString(keep, "matched") == 0) *flags = ACX_FILTER_KEEP_MATCHED;
    else if (PyUnicode_CompareWithASCIIString(keep, "unmatched") != 0) {
        PyErr_SetString(PyExc_ValueError, "keep must be 'unmatched' or 'matched'");
        return false;
    }
    return true;
}

// a new FilteredRows around f (filter_batch, filter_by_score_batch)
PyObject *filtered_object(acx_filtered_t *f, int device, uint64_t n_src, bool utf8) {
    OwnerObject *o = new_owner(RT_FILTERED_ROWS, f, device);
    if (o) {
        static_cast<FilteredRowsObject *>(o)->n_src = n_src;
        static_cast<FilteredRowsObject *>(o)->utf8 = utf8;
    }
    return reinterpret_cast<PyObject *>(o);
}

// filter_batch (no offset into a row is reported: the str class's search is on bytes too)
PyObject *filter_batch(PyObject *self, PyObject *args, PyObject *kwargs) {
    acx_automaton_t *a = ac_of(self);
    const bool utf8 = utf8_of(self);
    static const char *kw[] = {"haystacks", "overlapping", "keep", "min_matches", "offsets", "row_length", nullptr};
    PyObject *hay = nullptr, *ov = nullptr, *keep = nullptr, *mm = nullptr, *offsets = nullptr, *row_length = nullptr;
    int overlapping = 0;
    if (!PyArg_ParseTupleAndKeywords(args, kwargs, "O|O$OOOO:filter_batch", const_cast<char **>(kw), &hay, &ov, &keep, &mm,
                                     &offsets, &row_length))
        return nullptr;
    if (ov && !parse_bool(ov, "overlapping", &overlapping)) return nullptr;
    uint32_t flags = 0;
    if (keep && !parse_keep(keep, &flags)) return nullptr;
    unsigned long long min_matches = 1;
    if (mm) {
        long long v;
        int overflow;
        if (!parse_int(mm, "min_matches", &v, &overflow)) return nullptr;
        if (overflow < 0 || (!overflow && v < 1)) {
            PyErr_SetString(PyExc_ValueError, "min_matches must be at least 1");
            return nullptr;
        }
        min_matches = overflow ? ~0ull : (unsigned long long)v; // (more than any row can have)
    }
    const int device = acx_automaton_device(a);
    BatchInput in;
    if (!batch_input(hay, offsets, row_length, utf8, device, &in)) return nullptr;
    acx_filtered_t *f = nullptr;
    const int rc = batch_dispatch(
        device, in,
        [&](const uint8_t *p, uint64_t len, const uint64_t *off, uint64_t rows) {
            return acx_filter(a, p, len, off, rows, overlapping, min_matches, flags, &f);
        },
        [&](const uint8_t *p, uint64_t len, const uint64_t *d_off, uint64_t rows, uint64_t row_length) {
            return acx_filter_device(a, p, len, d_off, rows, row_length, overlapping, min_matches, flags, &f);
        });
    if (rc == BAD_OFFSETS) return nullptr;
    if (rc != ACX_OK) return raise_acx(rc);
    return filtered_object(f, device, in.rows, utf8);
}

// ---------------------------------------------------------------------------
// per-pattern weights: score_batch -> RowScores (acx_score / acx_score_device), filter_by_score_batch -> FilteredRows
// (acx_filter_scored / acx_filter_scored_device).  A RowScores owns the acx_scores_t; .score is a Column with the lifetime
// chain of a MatchColumns' columns.
// ---------------------------------------------------------------------------
// weights: one int per pattern, |w| < 2^31 -- an int64 / int32 buffer or a sequence of ints; sets the exception
bool parse_weights(PyObject *w, uint64_t n_patterns, std::vector<int32_t> *out) {
    std::vector<long long> wide;
    if (PyObject_CheckBuffer(w) && !PyBytes_Check(w) && !PyByteArray_Check(w)) {
        Py_buffer view;
        if (PyObject_GetBuffer(w, &view, PyBUF_FORMAT | PyBUF_C_CONTIGUOUS) < 0) return false;
        const char *f = view.format ? view.format : "B";
        if (*f == '@' || *f == '=' || *f == '<') f++;
        const bool i64 = (f[0] == 'q' || f[0] == 'l') && !f[1] && view.itemsize == 8;
        const bool i32 = (f[0] == 'i' || f[0] == 'l') && !f[1] && view.itemsize == 4;
        if (view.ndim != 1 || (!i64 && !i32)) {
            PyBuffer_Release(&view);
            PyErr_SetString(PyExc_TypeError, "argument 'weights': a buffer of weights must be 1-D int64 or int32");
            return false;
        }
        const size_t n = (size_t)(view.len / view.itemsize);
        wide.resize(n);
        for (size_t i = 0; i < n; i++)
            wide[i] = i64 ? (long long)static_cast<const int64_t *>(view.buf)[i] : (long long)static_cast<const int32_t *>(view.buf)[i];
        PyBuffer_Release(&view);
    } else {
        PyObject *seq = PyUnicode_Check(w) || PyBytes_Check(w) || PyByteArray_Check(w)
                            ? nullptr : PySequence_Fast(w, "argument 'weights': a sequence of ints or an int64 / int32 buffer is needed");
        if (!seq) {
            if (!PyErr_Occurred()) PyErr_SetString(PyExc_TypeError, "argument 'weights': a sequence of ints or an int64 / int32 buffer is needed");
            return false;
        }
        const Py_ssize_t n = PySequence_Fast_GET_SIZE(seq);
        wide.resize((size_t)n);
        for (Py_ssize_t i = 0; i < n; i++) {
            PyObject *it = PySequence_Fast_GET_ITEM(seq, i);
            if (PyBool_Check(it) || !PyIndex_Check(it)) {
                PyErr_Format(PyExc_TypeError, "argument 'weights': '%.100s' object cannot be interpreted as an integer", Py_TYPE(it)->tp_name);
                Py_DECREF(seq);
                return false;
            }
            PyObject *ix = PyNumber_Index(it);
            if (!ix) { Py_DECREF(seq); return false; }
            int overflow = 0;
            const long long v = PyLong_AsLongLongAndOverflow(ix, &overflow);
            Py_DECREF(ix);
            if (v == -1 && !overflow && PyErr_Occurred()) { Py_DECREF(seq); return false; }
            wide[(size_t)i] = overflow ? (overflow > 0 ? LLONG_MAX : LLONG_MIN) : v;
        }
        Py_DECREF(seq);
    }
    if (wide.size() != n_patterns) {
        PyErr_Format(PyExc_ValueError, "weights has %zu entries for %llu patterns: one per pattern is needed", wide.size(),
                     (unsigned long long)n_patterns);
        return false;
    }
    out->resize(wide.size());
    for (size_t i = 0; i < wide.size(); i++) {
        if (wide[i] > 2147483647LL || wide[i] < -2147483647LL) {
            PyErr_Format(PyExc_ValueError, "weights[%zu] is outside int32: |w| < 2^31 is needed", i);
            return false;
        }
        (*out)[i] = (int32_t)wide[i];
    }
    return true;
}

// score_batch (filter = false) and filter_by_score_batch (no offset into a row is reported: the str class's search is on
// bytes too)
template <bool filter> PyObject *scored(PyObject *self, PyObject *args, PyObject *kwargs) {
    acx_automaton_t *a = ac_of(self);
    const bool utf8 = utf8_of(self);
    static const char *kw_s[] = {"haystacks", "weights", "overlapping", "offsets", "row_length", nullptr};
    static const char *kw_f[] = {"haystacks", "weights", "overlapping", "keep", "min_score", "offsets", "row_length", nullptr};
    PyObject *hay = nullptr, *wts = nullptr, *ov = nullptr, *keep = nullptr, *ms = nullptr, *offsets = nullptr, *row_length = nullptr;
    int overlapping = 0;
    if (filter ? !PyArg_ParseTupleAndKeywords(args, kwargs, "OO|O$OOOO:filter_by_score_batch", const_cast<char **>(kw_f), &hay, &wts,
                                              &ov, &keep, &ms, &offsets, &row_length)
               : !PyArg_ParseTupleAndKeywords(args, kwargs, "OO|O$OO:score_batch", const_cast<char **>(kw_s), &hay, &wts, &ov, &offsets,
                                              &row_length))
        return nullptr;
    if (ov && !parse_bool(ov, "overlapping", &overlapping)) return nullptr;
    uint32_t flags = 0;
    if (keep && !parse_keep(keep, &flags)) return nullptr;
    long long min_score = 1;
    if (ms) {
        int overflow;
        if (!parse_int(ms, "min_score", &min_score, &overflow)) return nullptr;
        if (overflow) {
            PyErr_SetString(PyExc_ValueError, "min_score must fit an int64");
            return nullptr;
        }
    }
    acx_info_t info;
    if (acx_automaton_info(a, &info) != ACX_OK) return raise_acx(ACX_EINVAL);
    std::vector<int32_t> w;
    if (!parse_weights(wts, info.n_patterns, &w)) return nullptr;
    const int device = acx_automaton_device(a);
    BatchInput in;
    if (!batch_input(hay, offsets, row_length, utf8, device, &in)) return nullptr;
    acx_scores_t *s = nullptr;
    acx_filtered_t *f = nullptr;
    const int rc = batch_dispatch(
        device, in,
        [&](const uint8_t *p, uint64_t len, const uint64_t *off, uint64_t rows) {
            return filter ? acx_filter_scored(a, p, len, off, rows, overlapping, w.data(), w.size(), min_score, flags, &f)
                          : acx_score(a, p, len, off, rows, overlapping, w.data(), w.size(), &s);
        },
        [&](const uint8_t *p, uint64_t len, const uint64_t *d_off, uint64_t rows, uint64_t row_length) {
            return filter ? acx_filter_scored_device(a, p, len, d_off, rows, row_length, overlapping, w.data(), w.size(), min_score,
                                                     flags, &f)
                          : acx_score_device(a, p, len, d_off, rows, row_length, overlapping, w.data(), w.size(), &s);
        });
    if (rc == BAD_OFFSETS) return nullptr;
    if (rc != ACX_OK) return raise_acx(rc);
    if (!filter) return reinterpret_cast<PyObject *>(new_owner(RT_ROW_SCORES, s, device));
    return filtered_object(f, device, in.rows, utf8);
}

// ---------------------------------------------------------------------------
// the cover of a search's matches: mask_all / match_mask and their _batch forms -> str / bytes / MaskedRows (acx_mask /
// acx_mask_device).  A MaskedRows owns the acx_masked_t; .data (uint8) and .offsets (int64) are Columns with the lifetime
// chain of a MatchColumns' columns.
// ---------------------------------------------------------------------------

// fill: an int 0..255 or a one-byte buffer (the bytes class), a one-character ASCII str (the str class: the output stays
// valid UTF-8); sets the exception.  name: the argument as the messages call it (split_rows' delimiter takes the same check).
bool parse_fill(PyObject *fill, bool utf8, uint8_t *out, const char *name = "fill") {
    if (utf8) {
        if (!PyUnicode_Check(fill)) {
            PyErr_Format(PyExc_TypeError, "argument '%s': '%.100s' object cannot be converted to 'PyString'", name, Py_TYPE(fill)->tp_name);
            return false;
        }
        if (PyUnicode_GET_LENGTH(fill) != 1 || PyUnicode_READ_CHAR(fill, 0) > 0x7F) {
            PyErr_Format(PyExc_ValueError, "%s must be one ASCII character", name);
            return false;
        }
        *out = (uint8_t)PyUnicode_READ_CHAR(fill, 0);
        return true;
    }
    if (PyLong_Check(fill) && !PyBool_Check(fill)) {
        long long v;
        int overflow;
        if (!parse_int(fill, name, &v, &overflow)) return false;
        if (overflow || v < 0 || v > 255) {
            PyErr_Format(PyExc_ValueError, "%s must be in range(256)", name);
            return false;
        }
        *out = (uint8_t)v;
        return true;
    }
    if (PyUnicode_Check(fill) || PyBool_Check(fill) || !PyObject_CheckBuffer(fill)) {
        PyErr_Format(PyExc_TypeError, "argument '%s': an int in range(256) or a one-byte buffer is needed, not '%.100s'", name,
                     Py_TYPE(fill)->tp_name);
        return false;
    }
    Py_buffer v;
    if (!get_bytes_view(fill, &v)) return false;
    const bool one = v.len == 1;
    if (one) *out = *static_cast<const uint8_t *>(v.buf);
    PyBuffer_Release(&v);
    if (!one) PyErr_Format(PyExc_ValueError, "%s must be one byte", name);
    return one;
}

// the two argument checks and the per-character rule without an automaton (the CPU tests; module functions)
PyObject *mod_mask_fill(PyObject *, PyObject *args) {
    PyObject *fill = nullptr;
    int text = 0;
    if (!PyArg_ParseTuple(args, "Op:_mask_fill", &fill, &text)) return nullptr;
    uint8_t f = 0;
    if (!parse_fill(fill, text != 0, &f)) return nullptr;
    return PyLong_FromLong(f);
}
PyObject *mod_mask_per_character(PyObject *, PyObject *args) {
    PyObject *hay = nullptr;
    Py_buffer row;
    int text = 0;
    if (!PyArg_ParseTuple(args, "Uy*p:_mask_per_character", &hay, &row, &text)) return nullptr;
    Py_ssize_t len = 0;
    const char *p = PyUnicode_AsUTF8AndSize(hay, &len);
    PyObject *out = nullptr;
    if (p && row.len != len) PyErr_SetString(PyExc_ValueError, "row needs one entry per UTF-8 byte of haystack");
    else if (p) out = per_character(reinterpret_cast<const uint8_t *>(p), static_cast<const uint8_t *>(row.buf), (size_t)len, text != 0);
    PyBuffer_Release(&row);
    return out;
}

// mask_all / match_mask / mask_all_batch / match_mask_batch: text = the mask_all forms (the haystack with its matches
// filled), else the 0 / 1 mask; batch: the *_batch form.  No offset is reported: the str class's search is on bytes too.
template <bool text, bool batch> PyObject *mask(PyObject *self, PyObject *args, PyObject *kwargs) {
    acx_automaton_t *a = ac_of(self);
    const bool utf8 = utf8_of(self);
    static const char *kw_t[] = {"haystack", "fill", "overlapping", nullptr};
    static const char *kw_m[] = {"haystack", "overlapping", nullptr};
    static const char *kw_tb[] = {"haystacks", "fill", "overlapping", "offsets", "row_length", nullptr};
    static const char *kw_mb[] = {"haystacks", "overlapping", "offsets", "row_length", nullptr};
    PyObject *hay = nullptr, *fill_o = nullptr, *ov = nullptr, *offsets = nullptr, *row_length = nullptr;
    int overlapping = 0;
    if (batch ? (text ? !PyArg_ParseTupleAndKeywords(args, kwargs, "OO|O$OO:mask_all_batch", const_cast<char **>(kw_tb), &hay, &fill_o,
                                                     &ov, &offsets, &row_length)
                      : !PyArg_ParseTupleAndKeywords(args, kwargs, "O|O$OO:match_mask_batch", const_cast<char **>(kw_mb), &hay, &ov,
                                                     &offsets, &row_length))
              : (text ? !PyArg_ParseTupleAndKeywords(args, kwargs, "OO|O:mask_all", const_cast<char **>(kw_t), &hay, &fill_o, &ov)
                      : !PyArg_ParseTupleAndKeywords(args, kwargs, "O|O:match_mask", const_cast<char **>(kw_m), &hay, &ov)))
        return nullptr;
    if (ov && !parse_bool(ov, "overlapping", &overlapping)) return nullptr;
    uint8_t fill = 1;
    if (text && !parse_fill(fill_o, utf8, &fill)) return nullptr;
    const uint32_t flags = text ? 0 : ACX_MASK_ZERO;
    acx_masked_t *m = nullptr;
    int rc;
    if (!batch) {
        HaystackView v; // (a str or a buffer: these two take no tensor)
        if (!haystack_view(hay, utf8, false, -1, &v)) return nullptr;
        rc = nogil([&] { return acx_mask(a, v.p, v.len, nullptr, 1, overlapping, fill, flags, &m); });
        PyObject *out = nullptr;
        if (rc != ACX_OK) raise_acx(rc);
        else {
            const uint8_t *row = static_cast<const uint8_t *>(acx_masked_data(m)); // (a host result)
            out = !row ? raise_acx(ACX_EDEVICE)
                  : utf8 ? per_character(v.p, row, (size_t)v.len, text)
                         : PyBytes_FromStringAndSize(reinterpret_cast<const char *>(row), (Py_ssize_t)v.len);
        }
        acx_free_masked(m);
        return out;
    }
    const int device = acx_automaton_device(a);
    BatchInput in;
    if (!batch_input(hay, offsets, row_length, utf8, device, &in)) return nullptr;
    rc = batch_dispatch(
        device, in,
        [&](const uint8_t *p, uint64_t len, const uint64_t *off, uint64_t rows) {
            return acx_mask(a, p, len, off, rows, overlapping, fill, flags, &m);
        },
        [&](const uint8_t *p, uint64_t len, const uint64_t *d_off, uint64_t rows, uint64_t row_length) {
            return acx_mask_device(a, p, len, d_off, rows, row_length, overlapping, fill, flags, &m);
        });
    if (rc == BAD_OFFSETS) return nullptr;
    if (rc != ACX_OK) return raise_acx(rc);
    std::vector<uint8_t> *src = nullptr;
    if (utf8 && !in.tensor && !in.seq.all_ascii) {
        src = new (std::nothrow) std::vector<uint8_t>(std::move(in.seq.blob));
        if (!src) { acx_free_masked(m); return PyErr_NoMemory(); }
    }
    OwnerObject *o = new_owner(RT_MASKED_ROWS, m, device);
    if (!o) { delete src; return nullptr; }
    static_cast<MaskedRowsObject *>(o)->utf8 = utf8;
    static_cast<MaskedRowsObject *>(o)->text = text;
    static_cast<MaskedRowsObject *>(o)->src = src;
    return reinterpret_cast<PyObject *>(o);
}

// ---------------------------------------------------------------------------
// the merged spans of a search's matches: cover_spans / cover_spans_batch -> MatchSpans (acx_spans / acx_spans_device).  A
// MatchSpans owns the acx_spans_t; .start, .end and .row_offsets are Columns with the lifetime chain of a MatchColumns'
// columns.
// ---------------------------------------------------------------------------
// the check of `gap` without an automaton (the CPU tests; a module function)
PyObject *mod_spans_gap(PyObject *, PyObject *arg) { uint64_t g; return parse_u63(arg, "gap", &g) ? PyLong_FromUnsignedLongLong(g) : nullptr; }

// cover_spans / cover_spans_batch (code-point offsets when the str class's text is not ASCII)
template <bool batch> PyObject *spans(PyObject *self, PyObject *args, PyObject *kwargs) {
    acx_automaton_t *a = ac_of(self);
    const bool utf8 = utf8_of(self);
    static const char *kw_s[] = {"haystack", "overlapping", "gap", nullptr};
    static const char *kw_b[] = {"haystacks", "overlapping", "gap", "offsets", "row_length", nullptr};
    PyObject *hay = nullptr, *ov = nullptr, *gap_o = nullptr, *offsets = nullptr, *row_length = nullptr;
    int overlapping = 0;
    if (batch ? !PyArg_ParseTupleAndKeywords(args, kwargs, "O|O$OOO:cover_spans_batch", const_cast<char **>(kw_b), &hay, &ov, &gap_o,
                                             &offsets, &row_length)
              : !PyArg_ParseTupleAndKeywords(args, kwargs, "O|O$O:cover_spans", const_cast<char **>(kw_s), &hay, &ov, &gap_o))
        return nullptr;
    if (ov && !parse_bool(ov, "overlapping", &overlapping)) return nullptr;
    uint64_t gap = 0;
    if (gap_o && !parse_u63(gap_o, "gap", &gap)) return nullptr;
    const int device = acx_automaton_device(a);
    acx_spans_t *c = nullptr;
    int rc;
    if (batch) {
        BatchInput in;
        if (!batch_input(hay, offsets, row_length, utf8, device, &in)) return nullptr;
        const int codepoints = (utf8 && !in.tensor && !in.seq.all_ascii) ? 1 : 0;
        rc = batch_dispatch(
            device, in,
            [&](const uint8_t *p, uint64_t len, const uint64_t *off, uint64_t rows) {
                return acx_spans(a, p, len, off, rows, overlapping, codepoints, gap, &c);
            },
            [&](const uint8_t *p, uint64_t len, const uint64_t *d_off, uint64_t rows, uint64_t row_len) {
                return acx_spans_device(a, p, len, d_off, rows, row_len, overlapping, 0, gap, &c);
            });
        if (rc == BAD_OFFSETS) return nullptr;
    } else {
        HaystackView v;
        if (!haystack_view(hay, utf8, true, device, &v)) return nullptr;
        rc = single_dispatch(
            device, v,
            [&](const uint8_t *p, uint64_t len) { return acx_spans(a, p, len, nullptr, 0, overlapping, utf8 && !v.is_ascii, gap, &c); },
            [&](const uint8_t *p, uint64_t len) { return acx_spans_device(a, p, len, nullptr, 0, 0, overlapping, 0, gap, &c); }); // (merged where it lies)
    }
    if (rc != ACX_OK) return raise_acx(rc);
    OwnerObject *o = new_owner(RT_MATCH_SPANS, c, device);
    if (o) static_cast<MatchSpansObject *>(o)->batch = batch;
    return reinterpret_cast<PyObject *>(o);
}

// ---------------------------------------------------------------------------
// the matched text and its context: find_matches_as_snippets / find_matches_as_snippets_batch -> MatchSnippets (acx_snippets /
// acx_snippets_device).  A MatchSnippets owns the acx_snippets_t; its parts are Columns (.data uint8, the others int64) with
// the lifetime chain of a MatchColumns' columns.
// ---------------------------------------------------------------------------
// the check of `context` without an automaton (the CPU tests; a module function)
PyObject *mod_snippets_context(PyObject *, PyObject *arg) { uint64_t c; return parse_u63(arg, "context", &c) ? PyLong_FromUnsignedLongLong(c) : nullptr; }

// find_matches_as_snippets / _batch (the str class: UTF-8 bytes, the ends trimmed to characters).  The search runs on bytes:
// every offset of the result is a byte offset into .data
template <bool batch> PyObject *snippets(PyObject *self, PyObject *args, PyObject *kwargs) {
    acx_automaton_t *a = ac_of(self);
    const bool utf8 = utf8_of(self);
    static const char *kw_s[] = {"haystack", "overlapping", "context", nullptr};
    static const char *kw_b[] = {"haystacks", "overlapping", "context", "offsets", "row_length", nullptr};
    PyObject *hay = nullptr, *ov = nullptr, *ctx_o = nullptr, *offsets = nullptr, *row_length = nullptr;
    int overlapping = 0;
    if (batch ? !PyArg_ParseTupleAndKeywords(args, kwargs, "O|O$OOO:find_matches_as_snippets_batch", const_cast<char **>(kw_b), &hay,
                                             &ov, &ctx_o, &offsets, &row_length)
              : !PyArg_ParseTupleAndKeywords(args, kwargs, "O|O$O:find_matches_as_snippets", const_cast<char **>(kw_s), &hay, &ov, &ctx_o))
        return nullptr;
    if (ov && !parse_bool(ov, "overlapping", &overlapping)) return nullptr;
    uint64_t context = 0;
    if (ctx_o && !parse_u63(ctx_o, "context", &context)) return nullptr;
    const uint32_t flags = utf8 ? ACX_SNIPPET_UTF8 : 0;
    const int device = acx_automaton_device(a);
    acx_snippets_t *c = nullptr;
    int rc;
    if (batch) {
        BatchInput in;
        if (!batch_input(hay, offsets, row_length, utf8, device, &in)) return nullptr;
        rc = batch_dispatch(
            device, in,
            [&](const uint8_t *p, uint64_t len, const uint64_t *off, uint64_t rows) {
                return acx_snippets(a, p, len, off, rows, overlapping, context, flags, &c);
            },
            [&](const uint8_t *p, uint64_t len, const uint64_t *d_off, uint64_t rows, uint64_t row_len) {
                return acx_snippets_device(a, p, len, d_off, rows, row_len, overlapping, context, flags, &c);
            });
        if (rc == BAD_OFFSETS) return nullptr;
    } else {
        HaystackView v;
        if (!haystack_view(hay, utf8, true, device, &v)) return nullptr;
        rc = single_dispatch(
            device, v,
            [&](const uint8_t *p, uint64_t len) { return acx_snippets(a, p, len, nullptr, 0, overlapping, context, flags, &c); },
            [&](const uint8_t *p, uint64_t len) { return acx_snippets_device(a, p, len, nullptr, 0, 0, overlapping, context, flags, &c); }); // (cut where it lies)
    }
    if (rc != ACX_OK) return raise_acx(rc);
    OwnerObject *o = new_owner(RT_MATCH_SNIPPETS, c, device);
    if (o) {
        static_cast<MatchSnippetsObject *>(o)->batch = batch;
        static_cast<MatchSnippetsObject *>(o)->utf8 = utf8;
    }
    return reinterpret_cast<PyObject *>(o);
}

// ---------------------------------------------------------------------------
// whole words: find_whole_words_as_columns / _batch -> MatchColumns (acx_find_words / acx_find_words_device) and
// filter_whole_words_batch -> FilteredRows (acx_filter_words / acx_filter_words_device).  The search and the neighbour test
// run on bytes; the str class's offsets become character indexes here, on the host.
// ---------------------------------------------------------------------------
constexpr char ASCII_WORD_BYTES[] = "0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ_abcdefghijklmnopqrstuvwxyz";

// word_bytes: None (the default set: *set stays null) or any bytes-like of the byte values that count; sets the exception
bool parse_word_bytes(PyObject *o, uint8_t bits[32], const uint8_t **set) {
    *set = nullptr;
    if (!o || o == Py_None) return true;
    if (PyUnicode_Check(o)) {
        PyErr_SetString(PyExc_TypeError, "argument 'word_bytes': a bytes-like object of byte values is needed, not 'str'");
        return false;
    }
    Py_buffer view;
    if (!get_bytes_view(o, &view)) return false;
    std::memset(bits, 0, 32);
    const uint8_t *p = static_cast<const uint8_t *>(view.buf);
    for (Py_ssize_t i = 0; i < view.len; i++) bits[p[i] >> 3] |= (uint8_t)(1u << (p[i] & 7));
    PyBuffer_Release(&view);
    *set = bits;
    return true;
}

// the byte offsets of one row's matches [b, e) of a HOST result's columns to character indexes of the row's UTF-8 text: one
// pass over the row numbers its bytes, then every offset is looked up
bool to_characters(const uint8_t *row, uint64_t len, int64_t *start, int64_t *end, uint64_t b, uint64_t e) {
    if (b == e) return true;
    std::vector<int64_t> at;
    try {
        at.resize((size_t)len + 1);
    } catch (...) { PyErr_NoMemory(); return false; }
    int64_t chars = 0; // at[i] = the characters that begin before byte i (a match begins and ends between two characters)
    for (uint64_t i = 0; i < len; i++) {
        at[(size_t)i] = chars;
        if ((row[i] & 0xC0) != 0x80) chars++;
    }
    at[(size_t)len] = chars;
    for (uint64_t k = b; k < e; k++) {
        start[k] = at[(size_t)std::min<uint64_t>((uint64_t)start[k], len)];
        end[k] = at[(size_t)std::min<uint64_t>((uint64_t)end[k], len)];
    }
    return true;
}

// mode 0: find_whole_words_as_columns, 1: find_whole_words_as_columns_batch, 2: filter_whole_words_batch
template <int mode> PyObject *whole_words(PyObject *self, PyObject *args, PyObject *kwargs) {
    acx_automaton_t *a = ac_of(self);
    const bool utf8 = utf8_of(self);
    static const char *kw_s[] = {"haystack", "overlapping", "matchkind", "word_bytes", nullptr};
    static const char *kw_b[] = {"haystacks", "overlapping", "matchkind", "word_bytes", "offsets", "row_length", nullptr};
    static const char *kw_f[] = {"haystacks", "overlapping", "matchkind", "word_bytes", "keep", "min_matches", "offsets", "row_length", nullptr};
    PyObject *hay = nullptr, *ov = nullptr, *mk_o = nullptr, *wb = nullptr, *keep = nullptr, *mm = nullptr, *offsets = nullptr,
             *row_length = nullptr;
    if (mode == 0 ? !PyArg_ParseTupleAndKeywords(args, kwargs, "O|O$OO:find_whole_words_as_columns", const_cast<char **>(kw_s), &hay, &ov,
                                                 &mk_o, &wb)
        : mode == 1 ? !PyArg_ParseTupleAndKeywords(args, kwargs, "O|O$OOOO:find_whole_words_as_columns_batch", const_cast<char **>(kw_b),
                                                   &hay, &ov, &mk_o, &wb, &offsets, &row_length)
                    : !PyArg_ParseTupleAndKeywords(args, kwargs, "O|O$OOOOOO:filter_whole_words_batch", const_cast<char **>(kw_f), &hay,
                                                   &ov, &mk_o, &wb, &keep, &mm, &offsets, &row_length))
        return nullptr;
    int overlapping = 0, kind = ACX_MATCH_LEFTMOST_LONGEST;
    if (ov && !parse_bool(ov, "overlapping", &overlapping)) return nullptr;
    if (mk_o && !parse_matchkind(mk_o, &kind)) return nullptr;
    uint8_t bits[32];
    const uint8_t *set = nullptr;
    if (!parse_word_bytes(wb, bits, &set)) return nullptr;
    uint32_t flags = 0;
    if (keep && !parse_keep(keep, &flags)) return nullptr;
    unsigned long long min_matches = 1;
    if (mm) {
        long long v;
        int overflow;
        if (!parse_int(mm, "min_matches", &v, &overflow)) return nullptr;
        if (overflow < 0 || (!overflow && v < 1)) {
            PyErr_SetString(PyExc_ValueError, "min_matches must be at least 1");
            return nullptr;
        }
        min_matches = overflow ? ~0ull : (unsigned long long)v; // (more than any row can have)
    }
    const int device = acx_automaton_device(a);
    if (mode == 2) {
        BatchInput in;
        if (!batch_input(hay, offsets, row_length, utf8, device, &in)) return nullptr;
        acx_filtered_t *f = nullptr;
        const int rc = batch_dispatch(
            device, in,
            [&](const uint8_t *p, uint64_t len, const uint64_t *off, uint64_t rows) {
                return acx_filter_words(a, p, len, off, rows, overlapping, kind, set, min_matches, flags, &f);
            },
            [&](const uint8_t *p, uint64_t len, const uint64_t *d_off, uint64_t rows, uint64_t row_len) {
                return acx_filter_words_device(a, p, len, d_off, rows, row_len, overlapping, kind, set, min_matches, flags, &f);
            });
        if (rc == BAD_OFFSETS) return nullptr;
        if (rc != ACX_OK) return raise_acx(rc);
        return filtered_object(f, device, in.rows, utf8);
    }
    acx_columns_t *c = nullptr;
    int rc;
    bool converted = true;
    if (mode == 1) {
        BatchInput in;
        if (!batch_input(hay, offsets, row_length, utf8, device, &in)) return nullptr;
        rc = batch_dispatch(
            device, in,
            [&](const uint8_t *p, uint64_t len, const uint64_t *off, uint64_t rows) {
                return acx_find_words(a, p, len, off, rows, overlapping, kind, set, &c);
            },
            [&](const uint8_t *p, uint64_t len, const uint64_t *d_off, uint64_t rows, uint64_t row_len) {
                return acx_find_words_device(a, p, len, d_off, rows, row_len, overlapping, kind, set, &c);
            });
        if (rc == BAD_OFFSETS) return nullptr;
        if (rc == ACX_OK && utf8 && !in.tensor && !in.seq.all_ascii) { // a sequence of str: a host result, row by row
            int64_t *start = const_cast<int64_t *>(acx_columns_data(c, ACX_COL_START)), *end = const_cast<int64_t *>(acx_columns_data(c, ACX_COL_END));
            const int64_t *ro = acx_columns_data(c, ACX_COL_ROW_OFFSETS);
            for (uint64_t h = 0; converted && ro && h < in.rows; h++)
                converted = to_characters(in.seq.blob.data() + in.seq.off[(size_t)h], in.seq.off[(size_t)h + 1] - in.seq.off[(size_t)h], start, end,
                                          (uint64_t)ro[h], (uint64_t)ro[h + 1]);
        }
    } else {
        HaystackView v;
        if (!haystack_view(hay, utf8, true, device, &v)) return nullptr;
        rc = single_dispatch(
            device, v, [&](const uint8_t *p, uint64_t len) { return acx_find_words(a, p, len, nullptr, 0, overlapping, kind, set, &c); },
            [&](const uint8_t *p, uint64_t len) { return acx_find_words_device(a, p, len, nullptr, 0, 0, overlapping, kind, set, &c); });
        if (rc == ACX_OK && utf8 && !v.is_ascii)
            converted = to_characters(v.p, v.len, const_cast<int64_t *>(acx_columns_data(c, ACX_COL_START)),
                                      const_cast<int64_t *>(acx_columns_data(c, ACX_COL_END)), 0, acx_columns_count(c));
    }
    if (rc != ACX_OK) return raise_acx(rc);
    if (!converted) { acx_free_columns(c); return nullptr; }
    OwnerObject *o = new_owner(RT_MATCH_COLUMNS, c, device);
    if (o) static_cast<MatchColumnsObject *>(o)->batch = mode == 1;
    return reinterpret_cast<PyObject *>(o);
}

// ---------------------------------------------------------------------------
// a search's matches mapped onto token boundaries: label_tokens / label_tokens_batch -> TokenLabels (acx_tokens /
// acx_tokens_device).  A TokenLabels owns the acx_token_labels_t; .pattern and .begin are Columns with the lifetime chain of a
// MatchColumns' columns.  Tokens are a PARTITION here -- T + 1 boundaries, ts = tok, te = tok + 1; a (starts, ends) pair for
// tokenizers whose tokens leave gaps is the same C ABI with two arrays and is not bound yet.
// ---------------------------------------------------------------------------
// the characters of UTF-8 bytes: a byte that continues none begins one
uint64_t count_characters(const uint8_t *p, uint64_t n) {
    uint64_t k = 0;
    for (uint64_t i = 0; i < n; i++) k += (p[i] & 0xC0) != 0x80;
    return k;
}

// One haystack's LOCAL token boundaries: a sequence of ints or a 1-D contiguous int64 buffer of k + 1 entries that do not
// decrease and lie within 0 .. limit (the haystack's length in the unit at hand).  Sets the exception.
bool parse_boundaries(PyObject *o, uint64_t limit, std::vector<int64_t> *out) {
    out->clear();
    if (PyObject_CheckBuffer(o)) {
        Py_buffer view;
        if (PyObject_GetBuffer(o, &view, PyBUF_FULL_RO) < 0) return false;
        const char *fmt = view.format;
        if (fmt && (*fmt == '@' || *fmt == '=' || *fmt == '<')) fmt++;
        const bool ok = view.ndim == 1 && view.itemsize == 8 && fmt && (fmt[0] == 'q' || fmt[0] == 'l') && fmt[1] == 0 &&
                        PyBuffer_IsContiguous(&view, 'C');
        if (ok) out->assign(static_cast<const int64_t *>(view.buf), static_cast<const int64_t *>(view.buf) + view.len / 8);
        PyBuffer_Release(&view);
        if (!ok) {
            PyErr_SetString(PyExc_TypeError, "token_offsets: a buffer must be 1-D contiguous int64");
            return false;
        }
    } else {
        PyObject *seq = PySequence_Fast(o, "token_offsets must be a sequence of ints or an int64 buffer");
        if (!seq) return false;
        const Py_ssize_t n = PySequence_Fast_GET_SIZE(seq);
        out->reserve((size_t)n);
        for (Py_ssize_t i = 0; i < n; i++) {
            long long v;
            if (!parse_int(PySequence_Fast_GET_ITEM(seq, i), "token_offsets", &v)) { Py_DECREF(seq); return false; }
            out->push_back((int64_t)v);
        }
        Py_DECREF(seq);
    }
    if (out->empty()) {
        PyErr_SetString(PyExc_ValueError, "token_offsets needs tokens + 1 entries: at least one");
        return false;
    }
    bool ok = (*out)[0] >= 0 && (uint64_t)out->back() <= limit;
    for (size_t i = 0; ok && i + 1 < out->size(); i++) ok = (*out)[i] <= (*out)[i + 1];
    if (!ok) PyErr_SetString(PyExc_ValueError, "token_offsets must not decrease and must lie within 0 .. len(haystack)");
    return ok;
}

// local boundaries -> the tokens' global starts and ends, `base` positions into the data
void append_tokens(const std::vector<int64_t> &local, uint64_t base, std::vector<int64_t> *ts, std::vector<int64_t> *te) {
    for (size_t j = 0; j + 1 < local.size(); j++) {
        ts->push_back((int64_t)base + local[j]);
        te->push_back((int64_t)base + local[j + 1]);
    }
}

// The token_offsets tensor that goes with a haystack tensor: T + 1 boundaries where the haystack lies.
struct TokenTensor {
    PyObject *cap = nullptr;
    const int64_t *tok = nullptr;
    uint64_t T = 0;
    TokenTensor() = default;
    TokenTensor(const TokenTensor &) = delete;
    TokenTensor &operator=(const TokenTensor &) = delete;
    ~TokenTensor() { dlpack_release(cap); }
};
bool token_tensor(PyObject *o, bool on_device, int want_device, TokenTensor *t) {
    const uint64_t *words = nullptr;
    uint64_t entries = 0;
    if (!int64_tensor(o, "token_offsets", on_device, want_device, &t->cap, &words, &entries)) return false;
    if (entries < 1) {
        PyErr_SetString(PyExc_ValueError, "token_offsets needs tokens + 1 entries: at least one");
        return false;
    }
    t->tok = reinterpret_cast<const int64_t *>(words);
    t->T = entries - 1;
    return true;
}

// label_tokens / label_tokens_batch.  A tensor: global byte boundaries, tokens may cross rows.  A str, a buffer or a sequence
// of them: boundaries local to every haystack -- characters for the str class, the unit of find_matches_as_indexes and of a
// tokenizer's offset_mapping (the search reports code points and the library measures the rows in characters), else bytes.
template <bool batch> PyObject *label_tokens(PyObject *self, PyObject *args, PyObject *kwargs) {
    acx_automaton_t *a = ac_of(self);
    const bool utf8 = utf8_of(self);
    static const char *kw_s[] = {"haystack", "token_offsets", "overlapping", nullptr};
    static const char *kw_b[] = {"haystacks", "token_offsets", "overlapping", "offsets", "row_length", nullptr};
    PyObject *hay = nullptr, *tok_o = nullptr, *ov = nullptr, *offsets = nullptr, *row_length = nullptr;
    int overlapping = 0;
    if (batch ? !PyArg_ParseTupleAndKeywords(args, kwargs, "OO|O$OO:label_tokens_batch", const_cast<char **>(kw_b), &hay, &tok_o, &ov,
                                             &offsets, &row_length)
              : !PyArg_ParseTupleAndKeywords(args, kwargs, "OO|O:label_tokens", const_cast<char **>(kw_s), &hay, &tok_o, &ov))
        return nullptr;
    if (ov && !parse_bool(ov, "overlapping", &overlapping)) return nullptr;
    const int device = acx_automaton_device(a);
    acx_token_labels_t *l = nullptr;
    std::vector<int64_t> ts, te, local;
    std::unique_ptr<std::vector<int64_t>> ro;
    PyObject *inputs[3] = {nullptr, nullptr, nullptr}; // what a stage in flight still reads (TokenLabelsObject)
    auto keep = [&](PyObject **cap, int k) { inputs[k] = *cap; *cap = nullptr; };
    int rc;
    if (batch) {
        BatchInput in;
        if (!batch_input(hay, offsets, row_length, utf8, device, &in)) return nullptr;
        if (in.tensor) {
            TokenTensor t;
            if (!token_tensor(tok_o, in.on_device, device, &t)) return nullptr;
            rc = batch_dispatch(
                device, in,
                [&](const uint8_t *p, uint64_t len, const uint64_t *off, uint64_t rows) {
                    return acx_tokens(a, p, len, off, rows, overlapping, 0, t.tok, t.tok + 1, t.T, &l);
                },
                [&](const uint8_t *p, uint64_t len, const uint64_t *d_off, uint64_t rows, uint64_t row_len) {
                    return acx_tokens_device(a, p, len, d_off, rows, row_len, overlapping, t.tok, t.tok + 1, t.T, &l);
                });
            if (rc == BAD_OFFSETS) return nullptr;
            if (rc == ACX_OK && in.on_device) { keep(&in.cap, 0); keep(&in.cap_off, 1); keep(&t.cap, 2); }
        } else {
            PyObject *seq = PySequence_Fast(tok_o, "token_offsets must be a sequence with one entry per haystack");
            if (!seq) return nullptr;
            if ((uint64_t)PySequence_Fast_GET_SIZE(seq) != in.rows) {
                Py_DECREF(seq);
                PyErr_SetString(PyExc_ValueError, "token_offsets needs one entry per haystack");
                return nullptr;
            }
            const int codepoints = (utf8 && !in.seq.all_ascii) ? 1 : 0;
            ro.reset(new std::vector<int64_t>((size_t)in.rows + 1, 0));
            uint64_t base = 0;
            for (uint64_t h = 0; h < in.rows; h++) {
                const uint64_t b = in.seq.off[(size_t)h], e = in.seq.off[(size_t)h + 1];
                const uint64_t units = codepoints ? count_characters(in.seq.blob.data() + b, e - b) : e - b;
                if (!parse_boundaries(PySequence_Fast_GET_ITEM(seq, (Py_ssize_t)h), units, &local)) { Py_DECREF(seq); return nullptr; }
                append_tokens(local, base, &ts, &te);
                (*ro)[(size_t)h + 1] = (int64_t)ts.size();
                base += units;
            }
            Py_DECREF(seq);
            rc = nogil([&] {
                return acx_tokens(a, in.seq.blob.data(), in.seq.off[(size_t)in.rows], in.seq.off.data(), in.rows, overlapping, codepoints,
                                  ts.data(), te.data(), (uint64_t)ts.size(), &l);
            });
        }
    } else {
        HaystackView v;
        if (!haystack_view(hay, utf8, true, device, &v)) return nullptr;
        if (v.cap) {
            TokenTensor t;
            if (!token_tensor(tok_o, v.on_device, device, &t)) return nullptr;
            rc = single_dispatch(
                device, v,
                [&](const uint8_t *p, uint64_t len) { return acx_tokens(a, p, len, nullptr, 1, overlapping, 0, t.tok, t.tok + 1, t.T, &l); },
                [&](const uint8_t *p, uint64_t len) { return acx_tokens_device(a, p, len, nullptr, 0, 0, overlapping, t.tok, t.tok + 1, t.T, &l); });
            if (rc == ACX_OK && v.on_device) { keep(&v.cap, 0); keep(&t.cap, 2); }
        } else {
            const int codepoints = (utf8 && !v.is_ascii) ? 1 : 0;
            if (!parse_boundaries(tok_o, codepoints ? count_characters(v.p, v.len) : v.len, &local)) return nullptr;
            append_tokens(local, 0, &ts, &te);
            rc = nogil([&] { return acx_tokens(a, v.p, v.len, nullptr, 1, overlapping, codepoints, ts.data(), te.data(), (uint64_t)ts.size(), &l); });
        }
    }
    if (rc != ACX_OK) return raise_acx(rc);
    OwnerObject *o = new_owner(RT_TOKEN_LABELS, l, device); // (it frees l when the object cannot be made: the stage is waited for)
    if (!o) {
        for (PyObject *cap : inputs) dlpack_release(cap);
        return nullptr;
    }
    static_cast<TokenLabelsObject *>(o)->row_offsets = ro.release();
    for (int k = 0; k < 3; k++) static_cast<TokenLabelsObject *>(o)->inputs[k] = inputs[k];
    return reinterpret_cast<PyObject *>(o);
}

// ---------------------------------------------------------------------------
// the anchored search: match_at / match_prefix_batch -> MatchesAt (acx_match_at / acx_match_at_device).  No find runs.  A
// MatchesAt owns the acx_at_t; .pattern, .end and .row_offsets are Columns with the lifetime chain of a MatchColumns' columns.
// ---------------------------------------------------------------------------
// The positions of match_at on host data: a sequence of ints or a 1-D contiguous int64 buffer.  Their range is the C ABI's
// to check (ValueError: it knows the unit).  Sets the exception.
bool parse_positions(PyObject *o, std::vector<int64_t> *out) {
    out->clear();
    if (PyObject_CheckBuffer(o)) {
        Py_buffer view;
        if (PyObject_GetBuffer(o, &view, PyBUF_FULL_RO) < 0) return false;
        const char *fmt = view.format;
        if (fmt && (*fmt == '@' || *fmt == '=' || *fmt == '<')) fmt++;
        const bool ok = view.ndim == 1 && view.itemsize == 8 && fmt && (fmt[0] == 'q' || fmt[0] == 'l') && fmt[1] == 0 &&
                        PyBuffer_IsContiguous(&view, 'C');
        if (ok) out->assign(static_cast<const int64_t *>(view.buf), static_cast<const int64_t *>(view.buf) + view.len / 8);
        PyBuffer_Release(&view);
        if (!ok) PyErr_SetString(PyExc_TypeError, "positions: a buffer must be 1-D contiguous int64");
        return ok;
    }
    if (PyUnicode_Check(o)) {
        PyErr_SetString(PyExc_TypeError, "positions must be a sequence of ints or an int64 buffer");
        return false;
    }
    PyObject *seq = PySequence_Fast(o, "positions must be a sequence of ints or an int64 buffer");
    if (!seq) return false;
    const Py_ssize_t n = PySequence_Fast_GET_SIZE(seq);
    out->reserve((size_t)n);
    for (Py_ssize_t i = 0; i < n; i++) {
        long long v;
        int overflow = 0;
        if (!parse_int(PySequence_Fast_GET_ITEM(seq, i), "positions", &v, &overflow)) { Py_DECREF(seq); return false; }
        if (overflow) {
            Py_DECREF(seq);
            PyErr_SetString(PyExc_ValueError, "positions must lie within 0 .. len(haystack)");
            return false;
        }
        out->push_back((int64_t)v);
    }
    Py_DECREF(seq);
    return true;
}

// the MatchesAt around r; inputs: what a walk in flight still reads (released here when the object cannot be made)
PyObject *new_matches_at(acx_at_t *r, int device, PyObject *(&inputs)[3]) {
    OwnerObject *o = new_owner(RT_MATCHES_AT, r, device); // (it frees r when the object cannot be made: the walk is waited for)
    if (!o) {
        for (PyObject *cap : inputs) dlpack_release(cap);
        return nullptr;
    }
    for (int k = 0; k < 3; k++) static_cast<MatchesAtObject *>(o)->inputs[k] = inputs[k];
    return reinterpret_cast<PyObject *>(o);
}

// match_at(haystack, positions, overlapping=False, *, offsets=None, row_length=None).  A str or a buffer: positions on the
// host, in characters for the str class (ends as well).  A tensor: ONE int64 tensor of byte positions where it lies, and
// offsets / row_length cut it into rows as mask_all_batch takes them; in HBM everything stays there.
PyObject *match_at(PyObject *self, PyObject *args, PyObject *kwargs) {
    acx_automaton_t *a = ac_of(self);
    const bool utf8 = utf8_of(self);
    static const char *kw[] = {"haystack", "positions", "overlapping", "offsets", "row_length", nullptr};
    PyObject *hay = nullptr, *pos_o = nullptr, *ov = nullptr, *offsets = nullptr, *row_length = nullptr;
    int overlapping = 0;
    if (!PyArg_ParseTupleAndKeywords(args, kwargs, "OO|O$OO:match_at", const_cast<char **>(kw), &hay, &pos_o, &ov, &offsets, &row_length))
        return nullptr;
    if (ov && !parse_bool(ov, "overlapping", &overlapping)) return nullptr;
    if (offsets == Py_None) offsets = nullptr;
    if (row_length == Py_None) row_length = nullptr;
    const uint32_t flags = overlapping ? ACX_AT_OVERLAPPING : 0u;
    const int device = acx_automaton_device(a);
    acx_at_t *r = nullptr;
    PyObject *inputs[3] = {nullptr, nullptr, nullptr};
    auto keep = [&](PyObject **cap, int k) { inputs[k] = *cap; *cap = nullptr; };
    const uint64_t *words = nullptr;
    uint64_t n_pos = 0;
    PyObject *cap_pos = nullptr;
    int rc;
    if (offsets || row_length) { // ONE tensor cut into rows
        BatchInput in;
        if (utf8 || !batch_input(hay, offsets, row_length, utf8, device, &in)) {
            if (utf8) PyErr_SetString(PyExc_TypeError, "offsets / row_length cut ONE __dlpack__ tensor into rows: a str takes neither");
            return nullptr;
        }
        if (!int64_tensor(pos_o, "positions", in.on_device, device, &cap_pos, &words, &n_pos)) { dlpack_release(cap_pos); return nullptr; }
        const int64_t *pos = reinterpret_cast<const int64_t *>(words);
        rc = batch_dispatch(
            device, in,
            [&](const uint8_t *p, uint64_t len, const uint64_t *off, uint64_t rows) {
                return acx_match_at(a, p, len, off, rows, pos, n_pos, flags, 0, &r);
            },
            [&](const uint8_t *p, uint64_t len, const uint64_t *d_off, uint64_t rows, uint64_t row_len) {
                return acx_match_at_device(a, p, len, d_off, rows, row_len, pos, n_pos, flags, &r);
            });
        if (rc == ACX_OK && in.on_device) { keep(&in.cap, 0); keep(&in.cap_off, 1); keep(&cap_pos, 2); }
        dlpack_release(cap_pos);
        if (rc == BAD_OFFSETS) return nullptr;
    } else {
        HaystackView v;
        if (!haystack_view(hay, utf8, true, device, &v)) return nullptr;
        if (v.cap) {
            if (!int64_tensor(pos_o, "positions", v.on_device, device, &cap_pos, &words, &n_pos)) { dlpack_release(cap_pos); return nullptr; }
            const int64_t *pos = reinterpret_cast<const int64_t *>(words);
            rc = single_dispatch(
                device, v, [&](const uint8_t *p, uint64_t len) { return acx_match_at(a, p, len, nullptr, 1, pos, n_pos, flags, 0, &r); },
                [&](const uint8_t *p, uint64_t len) { return acx_match_at_device(a, p, len, nullptr, 0, 0, pos, n_pos, flags, &r); });
            if (rc == ACX_OK && v.on_device) { keep(&v.cap, 0); keep(&cap_pos, 2); }
            dlpack_release(cap_pos);
        } else {
            std::vector<int64_t> pos;
            if (!parse_positions(pos_o, &pos)) return nullptr;
            const int codepoints = (utf8 && !v.is_ascii) ? 1 : 0;
            rc = nogil([&] { return acx_match_at(a, v.p, v.len, nullptr, 1, pos.data(), (uint64_t)pos.size(), flags, codepoints, &r); });
        }
    }
    if (rc != ACX_OK) return raise_acx(rc);
    return new_matches_at(r, device, inputs);
}

// match_prefix_batch(haystacks, overlapping=False, *, full=False, offsets=None, row_length=None): the anchors are the rows
PyObject *match_prefix_batch(PyObject *self, PyObject *args, PyObject *kwargs) {
    acx_automaton_t *a = ac_of(self);
    const bool utf8 = utf8_of(self);
    static const char *kw[] = {"haystacks", "overlapping", "full", "offsets", "row_length", nullptr};
    PyObject *hay = nullptr, *ov = nullptr, *full_o = nullptr, *offsets = nullptr, *row_length = nullptr;
    int overlapping = 0, full = 0;
    if (!PyArg_ParseTupleAndKeywords(args, kwargs, "O|O$OOO:match_prefix_batch", const_cast<char **>(kw), &hay, &ov, &full_o, &offsets,
                                     &row_length))
        return nullptr;
    if (ov && !parse_bool(ov, "overlapping", &overlapping)) return nullptr;
    if (full_o && !parse_bool(full_o, "full", &full)) return nullptr;
    const uint32_t flags = ACX_AT_ROW_STARTS | (overlapping ? ACX_AT_OVERLAPPING : 0u) | (full ? ACX_AT_FULL : 0u);
    const int device = acx_automaton_device(a);
    BatchInput in;
    if (!batch_input(hay, offsets, row_length, utf8, device, &in)) return nullptr;
    const int codepoints = (!in.tensor && utf8 && !in.seq.all_ascii) ? 1 : 0;
    acx_at_t *r = nullptr;
    const int rc = batch_dispatch(
        device, in,
        [&](const uint8_t *p, uint64_t len, const uint64_t *off, uint64_t rows) {
            return acx_match_at(a, p, len, off, rows, nullptr, 0, flags, codepoints, &r);
        },
        [&](const uint8_t *p, uint64_t len, const uint64_t *d_off, uint64_t rows, uint64_t row_len) {
            return acx_match_at_device(a, p, len, d_off, rows, row_len, nullptr, 0, flags, &r);
        });
    if (rc == BAD_OFFSETS) return nullptr;
    if (rc != ACX_OK) return raise_acx(rc);
    PyObject *inputs[3] = {nullptr, nullptr, nullptr};
    if (in.on_device) { inputs[0] = in.cap; in.cap = nullptr; inputs[1] = in.cap_off; in.cap_off = nullptr; }
    return new_matches_at(r, device, inputs);
}

// ---------------------------------------------------------------------------
// greedy segmentation by the dictionary: segment / segment_batch -> Segments (acx_segment / acx_segment_device).  No find
// runs.  A Segments owns the acx_seg_t; its parts are Columns with the lifetime chain of a MatchColumns' columns.
// ---------------------------------------------------------------------------
// segment(haystack, *, utf8=None) / segment_batch(haystacks, *, utf8=None, offsets=None, row_length=None).  utf8: an unknown
// piece is a whole character (None: True for the str class, False for the bytes class).  A str is cut at characters and its
// boundaries are CHARACTER indexes; a tensor on the automaton's device stays in HBM end to end.
template <bool batch> PyObject *segment(PyObject *self, PyObject *args, PyObject *kwargs) {
    acx_automaton_t *a = ac_of(self);
    const bool str_class = utf8_of(self);
    static const char *kw_s[] = {"haystack", "utf8", nullptr};
    static const char *kw_b[] = {"haystacks", "utf8", "offsets", "row_length", nullptr};
    PyObject *hay = nullptr, *utf8_o = nullptr, *offsets = nullptr, *row_length = nullptr;
    if (batch ? !PyArg_ParseTupleAndKeywords(args, kwargs, "O|$OOO:segment_batch", const_cast<char **>(kw_b), &hay, &utf8_o, &offsets,
                                             &row_length)
              : !PyArg_ParseTupleAndKeywords(args, kwargs, "O|$O:segment", const_cast<char **>(kw_s), &hay, &utf8_o))
        return nullptr;
    int utf8 = str_class;
    if (utf8_o && utf8_o != Py_None && !parse_bool(utf8_o, "utf8", &utf8)) return nullptr;
    if (str_class && !utf8) {
        PyErr_SetString(PyExc_ValueError, "a str is cut at characters: utf8=False needs a BytesAhoCorasick");
        return nullptr;
    }
    const uint32_t flags = utf8 ? ACX_SEG_UTF8 : 0u;
    const int device = acx_automaton_device(a);
    acx_seg_t *r = nullptr;
    PyObject *inputs[3] = {nullptr, nullptr, nullptr};
    int rc;
    if (batch) {
        BatchInput in;
        if (!batch_input(hay, offsets, row_length, str_class, device, &in)) return nullptr;
        const int codepoints = (!in.tensor && str_class && !in.seq.all_ascii) ? 1 : 0;
        rc = batch_dispatch(
            device, in,
            [&](const uint8_t *p, uint64_t len, const uint64_t *off, uint64_t rows) {
                return acx_segment(a, p, len, off, rows, flags, codepoints, &r);
            },
            [&](const uint8_t *p, uint64_t len, const uint64_t *d_off, uint64_t rows, uint64_t row_len) {
                return acx_segment_device(a, p, len, d_off, rows, row_len, flags, &r);
            });
        if (rc == BAD_OFFSETS) return nullptr;
        if (rc == ACX_OK && in.on_device) { inputs[0] = in.cap; in.cap = nullptr; inputs[1] = in.cap_off; in.cap_off = nullptr; }
    } else {
        HaystackView v;
        if (!haystack_view(hay, str_class, true, device, &v)) return nullptr;
        if (v.cap && capsule_tensor(v.cap).ndim != 1) {
            PyErr_SetString(PyExc_TypeError, "Only one-dimensional sequences are supported");
            return nullptr;
        }
        const int codepoints = (str_class && !v.is_ascii) ? 1 : 0;
        rc = single_dispatch(
            device, v, [&](const uint8_t *p, uint64_t len) { return acx_segment(a, p, len, nullptr, 1, flags, codepoints, &r); },
            [&](const uint8_t *p, uint64_t len) { return acx_segment_device(a, p, len, nullptr, 0, 0, flags, &r); });
        if (rc == ACX_OK && v.on_device) { inputs[0] = v.cap; v.cap = nullptr; }
    }
    if (rc != ACX_OK) return raise_acx(rc);
    OwnerObject *o = new_owner(RT_SEGMENTS, r, device); // (it frees r when the object cannot be made: the stage is waited for)
    if (!o) {
        for (PyObject *cap : inputs) dlpack_release(cap);
        return nullptr;
    }
    static_cast<SegmentsObject *>(o)->batch = batch;
    for (int k = 0; k < 3; k++) static_cast<SegmentsObject *>(o)->inputs[k] = inputs[k];
    return reinterpret_cast<PyObject *>(o);
}

// ---------------------------------------------------------------------------
// WordPiece tokenization by the dictionary: wordpiece / wordpiece_batch -> WordPieces (acx_wordpiece / acx_wordpiece_device).
// No find runs.  A WordPieces owns the acx_wp_t; its parts are Columns with the lifetime chain of a MatchColumns' columns.
// ---------------------------------------------------------------------------
constexpr char ASCII_WHITESPACE[] = " \t\n\r\x0b\x0c";
constexpr char ASCII_PUNCTUATION[] = "!\"#$%&'()*+,-./:;<=>?@[\\]^_`{|}~";

struct WordPieceArgs {
    uint8_t cls[256];
    std::string prefix;
    uint64_t max_word = 100;
    int64_t unk_id = -1;
};

// a set of byte values or the continuation prefix: None (the default), a bytes-like or -- the str class -- a str, which for
// a set must be ASCII (a UTF-8 character is never split); sets the exception
bool parse_wp_bytes(PyObject *o, const char *name, bool str_class, bool ascii_only, const char *dflt, std::string *out) {
    if (!o || o == Py_None) { *out = dflt; return true; }
    if (PyUnicode_Check(o)) {
        if (!str_class) {
            PyErr_Format(PyExc_TypeError, "argument '%s': a bytes-like object is needed, not 'str'", name);
            return false;
        }
        if (ascii_only && !PyUnicode_IS_ASCII(o)) {
            PyErr_Format(PyExc_ValueError, "%s must be ASCII: a UTF-8 character is never split", name);
            return false;
        }
        Py_ssize_t len;
        const char *s = PyUnicode_AsUTF8AndSize(o, &len);
        if (!s) return false;
        out->assign(s, (size_t)len);
        return true;
    }
    Py_buffer view;
    if (!get_bytes_view(o, &view)) return false;
    out->assign(static_cast<const char *>(view.buf), (size_t)view.len);
    PyBuffer_Release(&view);
    return true;
}

// the keyword arguments of wordpiece / wordpiece_batch (each may be null or None: its default); sets the exception
bool parse_wordpiece_args(bool str_class, PyObject *prefix, PyObject *separators, PyObject *isolated, PyObject *max_word,
                          PyObject *unk_id, WordPieceArgs *A) {
    std::string sep, alone;
    if (!parse_wp_bytes(prefix, "continuation_prefix", str_class, false, "##", &A->prefix)) return false;
    if (!parse_wp_bytes(separators, "separators", str_class, true, ASCII_WHITESPACE, &sep)) return false;
    if (!parse_wp_bytes(isolated, "isolated", str_class, true, "", &alone)) return false;
    std::memset(A->cls, ACX_WP_WORD, 256);
    for (const char c : sep) A->cls[(uint8_t)c] = ACX_WP_SPACE;
    for (const char c : alone) {
        if (A->cls[(uint8_t)c] == ACX_WP_SPACE) {
            PyErr_Format(PyExc_ValueError, "byte value %d is in separators and in isolated", (int)(uint8_t)c);
            return false;
        }
        A->cls[(uint8_t)c] = ACX_WP_ALONE;
    }
    if (max_word && max_word != Py_None) {
        long long v;
        int overflow;
        if (!parse_int(max_word, "max_word_bytes", &v, &overflow)) return false;
        if (overflow || v < 1 || v > (long long)ACX_WP_MAX_WORD) {
            PyErr_Format(PyExc_ValueError, "max_word_bytes must be in range(1, %u)", ACX_WP_MAX_WORD + 1);
            return false;
        }
        A->max_word = (uint64_t)v;
    }
    if (unk_id && unk_id != Py_None) {
        long long v;
        int overflow;
        if (!parse_int(unk_id, "unk_id", &v, &overflow)) return false;
        if (overflow) {
            PyErr_SetString(PyExc_ValueError, "unk_id must be in range(-2**63, 2**63)");
            return false;
        }
        A->unk_id = (int64_t)v;
    }
    return true;
}

// the checks above without an automaton (the CPU tests; a module function): (cls, prefix, max_word_bytes, unk_id)
PyObject *mod_wordpiece_args(PyObject *, PyObject *args) {
    PyObject *utf8 = nullptr, *prefix = nullptr, *sep = nullptr, *alone = nullptr, *max_word = nullptr, *unk_id = nullptr;
    if (!PyArg_ParseTuple(args, "O|OOOOO:_wordpiece_args", &utf8, &prefix, &sep, &alone, &max_word, &unk_id)) return nullptr;
    WordPieceArgs A;
    if (!parse_wordpiece_args(PyObject_IsTrue(utf8) == 1, prefix, sep, alone, max_word, unk_id, &A)) return nullptr;
    return Py_BuildValue("(y#y#KL)", reinterpret_cast<const char *>(A.cls), (Py_ssize_t)256, A.prefix.data(), (Py_ssize_t)A.prefix.size(),
                         (unsigned long long)A.max_word, (long long)A.unk_id);
}

// the row begins of a host batch in the result's unit: bytes, or -- chars -- the characters that begin before each
std::vector<int64_t> *host_row_begins(const uint8_t *p, const uint64_t *off, uint64_t rows, bool chars) {
    std::vector<int64_t> *b = new (std::nothrow) std::vector<int64_t>();
    if (!b) return nullptr;
    try {
        b->resize((size_t)rows + 1);
    } catch (...) { delete b; return nullptr; }
    uint64_t at = 0, n = 0;
    for (uint64_t r = 0; r <= rows; r++) {
        if (chars)
            for (; at < off[r]; at++) n += (p[at] & 0xC0) != 0x80;
        (*b)[(size_t)r] = (int64_t)(chars ? n : off[r]);
    }
    return b;
}

// wordpiece(haystack, *, continuation_prefix="##", separators=None, isolated=None, max_word_bytes=100, unk_id=-1) /
// wordpiece_batch(haystacks, *, ..., offsets=None, row_length=None).  A str's positions are CHARACTER indexes (the host route);
// a tensor on the automaton's device stays in HBM end to end.
template <bool batch> PyObject *wordpiece(PyObject *self, PyObject *args, PyObject *kwargs) {
    acx_automaton_t *a = ac_of(self);
    const bool str_class = utf8_of(self);
    static const char *kw_s[] = {"haystack", "continuation_prefix", "separators", "isolated", "max_word_bytes", "unk_id", nullptr};
    static const char *kw_b[] = {"haystacks", "continuation_prefix", "separators", "isolated", "max_word_bytes", "unk_id", "offsets",
                                 "row_length", nullptr};
    PyObject *hay = nullptr, *prefix = nullptr, *sep = nullptr, *alone = nullptr, *max_word = nullptr, *unk_id = nullptr,
             *offsets = nullptr, *row_length = nullptr;
    if (batch ? !PyArg_ParseTupleAndKeywords(args, kwargs, "O|$OOOOOOO:wordpiece_batch", const_cast<char **>(kw_b), &hay, &prefix, &sep,
                                             &alone, &max_word, &unk_id, &offsets, &row_length)
              : !PyArg_ParseTupleAndKeywords(args, kwargs, "O|$OOOOO:wordpiece", const_cast<char **>(kw_s), &hay, &prefix, &sep, &alone,
                                             &max_word, &unk_id))
        return nullptr;
    WordPieceArgs A;
    if (!parse_wordpiece_args(str_class, prefix, sep, alone, max_word, unk_id, &A)) return nullptr;
    const uint8_t *pre = reinterpret_cast<const uint8_t *>(A.prefix.data());
    const uint64_t pre_len = A.prefix.size();
    const int device = acx_automaton_device(a);
    acx_wp_t *r = nullptr;
    PyObject *inputs[3] = {nullptr, nullptr, nullptr};
    std::vector<int64_t> *row_begin = nullptr;
    uint64_t row_len_kept = 0;
    const uint64_t *d_off_kept = nullptr;
    int rc;
    if (batch) {
        BatchInput in;
        if (!batch_input(hay, offsets, row_length, str_class, device, &in)) return nullptr;
        const int codepoints = (!in.tensor && str_class && !in.seq.all_ascii) ? 1 : 0;
        bool no_memory = false;
        rc = batch_dispatch(
            device, in,
            [&](const uint8_t *p, uint64_t len, const uint64_t *off, uint64_t rows) {
                row_begin = host_row_begins(p, off, rows, codepoints != 0);
                if (!row_begin) { no_memory = true; return (int)ACX_ENOMEM; }
                return acx_wordpiece(a, p, len, off, rows, A.cls, pre, pre_len, A.max_word, A.unk_id, 0, codepoints, &r);
            },
            [&](const uint8_t *p, uint64_t len, const uint64_t *d_off, uint64_t rows, uint64_t row_len) {
                row_len_kept = row_len;
                d_off_kept = d_off;
                return acx_wordpiece_device(a, p, len, d_off, rows, row_len, A.cls, pre, pre_len, A.max_word, A.unk_id, 0, &r);
            });
        if (rc == BAD_OFFSETS) return nullptr;
        if (no_memory) return PyErr_NoMemory();
        if (rc == ACX_OK && in.on_device) { inputs[0] = in.cap; in.cap = nullptr; inputs[1] = in.cap_off; in.cap_off = nullptr; }
    } else {
        HaystackView v;
        if (!haystack_view(hay, str_class, true, device, &v)) return nullptr;
        if (v.cap && capsule_tensor(v.cap).ndim != 1) {
            PyErr_SetString(PyExc_TypeError, "Only one-dimensional sequences are supported");
            return nullptr;
        }
        const int codepoints = (str_class && !v.is_ascii) ? 1 : 0;
        rc = single_dispatch(
            device, v,
            [&](const uint8_t *p, uint64_t len) {
                return acx_wordpiece(a, p, len, nullptr, 1, A.cls, pre, pre_len, A.max_word, A.unk_id, 0, codepoints, &r);
            },
            [&](const uint8_t *p, uint64_t len) {
                return acx_wordpiece_device(a, p, len, nullptr, 0, 0, A.cls, pre, pre_len, A.max_word, A.unk_id, 0, &r);
            });
        if (rc == ACX_OK && v.on_device) { inputs[0] = v.cap; v.cap = nullptr; }
    }
    if (rc != ACX_OK) { delete row_begin; return raise_acx(rc); }
    OwnerObject *o = new_owner(RT_WORD_PIECES, r, device); // (it frees r when the object cannot be made: the stage is waited for)
    if (!o) {
        delete row_begin;
        for (PyObject *cap : inputs) dlpack_release(cap);
        return nullptr;
    }
    WordPiecesObject *w = static_cast<WordPiecesObject *>(o);
    w->batch = batch;
    w->row_begin = row_begin;
    w->row_length = row_len_kept;
    w->d_off = d_off_kept;
    for (int k = 0; k < 3; k++) w->inputs[k] = inputs[k];
    return reinterpret_cast<PyObject *>(o);
}

// ---------------------------------------------------------------------------
// split_rows(data, delimiter=b"\n") -> RowOffsets (acx_split_rows / acx_split_rows_device): a delimited buffer cut into rows.
// A module function -- no automaton is involved.  A RowOffsets owns the acx_rows_t; .offsets is a Column with the lifetime
// chain of a MatchColumns' columns, and what the _batch methods take as offsets=.
// ---------------------------------------------------------------------------
PyObject *mod_split_rows(PyObject *, PyObject *args, PyObject *kwargs) {
    static const char *kw[] = {"data", "delimiter", nullptr};
    PyObject *data = nullptr, *delim = nullptr;
    if (!PyArg_ParseTupleAndKeywords(args, kwargs, "O|O:split_rows", const_cast<char **>(kw), &data, &delim)) return nullptr;
    uint8_t d = '\n';
    if (delim && !parse_fill(delim, PyUnicode_Check(delim) != 0, &d, "delimiter")) return nullptr;
    HaystackView v; // (a tensor on any device)
    if (!haystack_view(data, false, true, -1, &v)) return nullptr;
    if (v.cap && capsule_tensor(v.cap).ndim != 1) {
        PyErr_SetString(PyExc_TypeError, "Only one-dimensional sequences are supported");
        return nullptr;
    }
    acx_rows_t *r = nullptr;
    const int rc = single_dispatch(
        v.cap ? capsule_tensor(v.cap).device.device_id : 0, v,
        [&](const uint8_t *p, uint64_t len) { return acx_split_rows(p, len, d, &r); },
        [&](const uint8_t *p, uint64_t len) { return acx_split_rows_device(p, len, d, &r); });
    if (rc != ACX_OK) return raise_acx(rc);
    return reinterpret_cast<PyObject *>(new_owner(RT_ROW_OFFSETS, r, acx_rows_device(r)));
}

// ---------------------------------------------------------------------------
// the matches themselves: find_matches_as_indexes, find_matches_as_strings, replace_all
// ---------------------------------------------------------------------------
// src/lib.rs:229-249 (the str class: code-point offsets) and 422-434 (the bytes class: byte offsets, no fix-up).  A tensor in
// HBM is searched where it lies; the records come back with ONE D2H copy of the result.
PyObject *find_indexes(PyObject *self, PyObject *args, PyObject *kwargs) {
    acx_automaton_t *a = ac_of(self);
    PyObject *hay; int overlapping;
    if (!parse_find_args(args, kwargs, "O|O:find_matches_as_indexes", &hay, &overlapping)) return nullptr;
    HaystackView v;
    if (!haystack_view(hay, utf8_of(self), true, acx_automaton_device(a), &v)) return nullptr;
    acx_match_t *m = nullptr; uint64_t n = 0; // a host haystack's matches; a tensor's: dm
    std::vector<acx_match_t> dm;
    const int rc = single_dispatch(
        acx_automaton_device(a), v,
        // (an ASCII str: byte offset == code-point index, the device fix-up is skipped)
        [&](const uint8_t *p, uint64_t len) { return acx_find(a, p, len, overlapping, utf8_of(self) && !v.is_ascii, &m, &n); },
        [&](const uint8_t *p, uint64_t len) {
            acx_result_t *r = nullptr;
            int rc = acx_find_device(a, p, len, nullptr, 0, 0, overlapping, 0, &r);
            if (rc == ACX_OK) {
                dm.resize((size_t)acx_result_count(r));
                if (!dm.empty()) rc = acx_result_copy(r, dm.data());
            }
            if (r) acx_free_result(r);
            return rc;
        });
    if (rc != ACX_OK) return raise_acx(rc);
    PyObject *list = v.on_device ? matches_to_list(dm.data(), (uint64_t)dm.size()) : matches_to_list(m, n);
    acx_free_matches(m);
    return list;
}

// src/lib.rs:253-272 (the str class alone)
PyObject *ac_find_strings(PyObject *self, PyObject *args, PyObject *kwargs) {
    PyObject *hay; int overlapping;
    if (!parse_find_args(args, kwargs, "O|O:find_matches_as_strings", &hay, &overlapping)) return nullptr;
    HaystackView v;
    if (!haystack_view(hay, true, false, -1, &v)) return nullptr;
    acx_match_t *m = nullptr; uint64_t n = 0;
    const int rc = nogil([&] { return acx_find(ac_of(self), v.p, v.len, overlapping, 0 /* byte offsets */, &m, &n); });
    if (rc != ACX_OK) return raise_acx(rc);
    PyObject *patterns = reinterpret_cast<AcObject *>(self)->patterns;
    PyObject *list = list_of(0, n, [&](uint64_t i) -> PyObject * {
        if (!patterns) // slice of the haystack by byte offsets, src/lib.rs:267-270
            return PyUnicode_DecodeUTF8(reinterpret_cast<const char *>(v.p) + m[i].start, (Py_ssize_t)(m[i].end - m[i].start), "strict");
        PyObject *item = PyList_GET_ITEM(patterns, (Py_ssize_t)m[i].pattern); // clone_ref of the stored pattern, src/lib.rs:263-266
        Py_INCREF(item);
        return item;
    });
    acx_free_matches(m);
    return list;
}

// replace_all: the str class's str, or the bytes class's buffer or tensor (searched and spliced where it lies; only the
// output crosses to the host).  The haystack is looked at before replace_with.
PyObject *replace_all(PyObject *self, PyObject *args, PyObject *kwargs) {
    static const char *kw[] = {"haystack", "replace_with", nullptr};
    PyObject *hay, *rw;
    if (!PyArg_ParseTupleAndKeywords(args, kwargs, "OO:replace_all", const_cast<char **>(kw), &hay, &rw)) return nullptr;
    acx_automaton_t *a = ac_of(self);
    const bool utf8 = utf8_of(self);
    HaystackView v;
    if (!haystack_view(hay, utf8, true, acx_automaton_device(a), &v)) return nullptr;
    std::vector<uint8_t> blob;
    std::vector<uint64_t> off;
    if (!replacements(rw, utf8, &blob, &off)) return nullptr;
    acx_replaced_t *r = nullptr;
    const int rc = single_dispatch(
        acx_automaton_device(a), v,
        [&](const uint8_t *p, uint64_t len) { return acx_replace(a, p, len, nullptr, 0, blob.data(), off.data(), off.size() - 1, &r); },
        [&](const uint8_t *p, uint64_t len) { return acx_replace_device(a, p, len, nullptr, 0, 0, blob.data(), off.data(), off.size() - 1, &r); });
    if (rc != ACX_OK) return raise_acx(rc);
    return replaced_result(r, utf8);
}

// ---------------------------------------------------------------------------
// the method tables: the methods both classes have, once; what only one has, or has with words of its own, in front
// ---------------------------------------------------------------------------
#define KW(...) reinterpret_cast<PyCFunction>(reinterpret_cast<void (*)()>(__VA_ARGS__)), METH_VARARGS | METH_KEYWORDS
const PyMethodDef SHARED_METHODS[] = {
    {"find_matches_as_indexes", KW(find_indexes),
     "Return matches as tuple of (index_into_patterns, start_index_in_haystack, "
     "end_index_in_haystack). If ``overlapping`` is ``False`` (the default), don't include "
     "overlapping results."},
    {"find_matches_as_indexes_batch", KW(find_batch),
     "[extension] one device pass over many haystacks; equals "
     "[self.find_matches_as_indexes(h, overlapping) for h in haystacks].  devices=[ordinals]: the batch "
     "is cut into contiguous ranges of haystacks, one per device (replicas of the automaton are built on "
     "first use), scanned side by side from one host thread each."},
    {"replace_all_batch", KW(replace_all_batch), "[extension] [self.replace_all(h, replace_with) for h in haystacks] in one call."},
    {"_info", automaton_info, METH_NOARGS, "[extension] automaton / device facts as a dict."},
    {"is_match", KW(summary<SUM_IS_MATCH, false>),
     "[extension] bool(find_matches_as_indexes(haystack)) without the match list (the crate's is_match).  No early exit: "
     "one search over the whole haystack."},
    {"find_first", KW(summary<SUM_FIND_FIRST, false>),
     "[extension] find_matches_as_indexes(haystack)[0], or None (the crate's find for the object's match kind)."},
    {"count_matches", KW(summary<SUM_COUNT, false>), "[extension] len(find_matches_as_indexes(haystack, overlapping))."},
    {"count_by_pattern", KW(summary<SUM_BY_PATTERN, false>),
     "[extension] one int per pattern: how many of find_matches_as_indexes(haystack, overlapping) name it."},
    {"is_match_batch", KW(summary<SUM_IS_MATCH, true>), "[extension] [self.is_match(h) for h in haystacks] in one call."},
    {"find_first_batch", KW(summary<SUM_FIND_FIRST, true>), "[extension] [self.find_first(h) for h in haystacks] in one call."},
    {"count_matches_batch", KW(summary<SUM_COUNT, true>), "[extension] [self.count_matches(h, overlapping) for h in haystacks] in one call."},
    {"count_by_pattern_batch", KW(summary<SUM_BY_PATTERN, true>),
     "[extension] the per-pattern totals over all haystacks: the sum of self.count_by_pattern(h, overlapping)."},
    {"count_by_pattern_sparse_batch", KW(sparse_counts),
     "[extension] count_by_pattern_sparse_batch(haystacks, overlapping=False, *, offsets=None, row_length=None) -> "
     "PatternCounts: which patterns occur in which haystack and how often, as a CSR matrix of len(haystacks) x patterns "
     "(row_offsets, pattern ascending within a row, count: int64 Columns that torch.sparse_csr_tensor takes as they are).  "
     "haystacks: a sequence, as in every other _batch method, or ONE 1-D contiguous uint8 __dlpack__ tensor that holds the "
     "rows back to back, cut by exactly one of offsets (a 1-D int64 __dlpack__ tensor of rows + 1 entries on the haystack's "
     "device) and row_length (an int that divides the tensor's length).  A tensor on the automaton's device is searched and "
     "reduced there and the result stays there; nothing but its size crosses the bus."},
    {"filter_batch", KW(filter_batch),
     "[extension] filter_batch(haystacks, overlapping=False, *, keep='unmatched', min_matches=1, offsets=None, "
     "row_length=None) -> FilteredRows: the rows of the batch with fewer than min_matches matches (keep='unmatched': drop "
     "every row that contains a pattern) or with at least that many (keep='matched'), compacted where the search ran: "
     ".rows (the kept source row indexes), .offsets and .data (the kept rows' own bytes back to back).  haystacks: a "
     "sequence, or ONE 1-D contiguous uint8 __dlpack__ tensor cut by exactly one of offsets and row_length, as for "
     "count_by_pattern_sparse_batch.  A tensor on the automaton's device is searched and compacted there and the result "
     "stays there; nothing but its two sizes crosses the bus."},
    {"score_batch", KW(scored<false>),
     "[extension] score_batch(haystacks, weights, overlapping=False, *, offsets=None, row_length=None) -> RowScores: for "
     "every row the sum of weights[pattern] over the matches find_matches_as_indexes_batch reports for it (int64; it wraps "
     "modulo 2^64).  weights: one int per pattern, |w| < 2^31 -- a sequence of ints or an int64 / int32 buffer.  haystacks: "
     "a sequence, or ONE 1-D contiguous uint8 __dlpack__ tensor cut by exactly one of offsets and row_length, as for "
     "count_by_pattern_sparse_batch.  A tensor on the automaton's device is searched and scored there and the result stays "
     "there."},
    {"filter_by_score_batch", KW(scored<true>),
     "[extension] filter_by_score_batch(haystacks, weights, overlapping=False, *, keep='unmatched', min_score=1, "
     "offsets=None, row_length=None) -> FilteredRows: filter_batch with the verdict on a row taken from its score -- a row "
     "is matched when score_batch's value for it is at least min_score (any int64)."},
    {"mask_all", KW(mask<true, false>),
     "[extension] mask_all(haystack, fill, overlapping=False) -> the haystack with every byte that a match covers replaced "
     "by fill and every other byte where it was: fixed-fill redaction.  fill: an int 0..255 or a one-byte buffer "
     "(BytesAhoCorasick), a one-character ASCII str (AhoCorasick: a covered character becomes ONE fill, so the result has "
     "len(haystack) characters).  overlapping=True on a Standard object covers the union of all occurrences."},
    {"match_mask", KW(mask<false, false>),
     "[extension] match_mask(haystack, overlapping=False) -> bytes: 1 where a match covers the haystack's byte "
     "(AhoCorasick: its character), else 0; len(haystack) entries."},
    {"mask_all_batch", KW(mask<true, true>),
     "[extension] mask_all_batch(haystacks, fill, overlapping=False, *, offsets=None, row_length=None) -> MaskedRows: "
     "mask_all of every row in one call, as one uint8 .data in the input's own layout with its .offsets.  haystacks: a "
     "sequence, or ONE 1-D contiguous uint8 __dlpack__ tensor cut by exactly one of offsets and row_length, as for "
     "count_by_pattern_sparse_batch.  A tensor on the automaton's device is searched and painted there and the result "
     "stays there.  AhoCorasick: .data is in UTF-8 bytes (a covered k-byte character is k fills); tolist() gives one fill "
     "per character for a sequence of str and the bytes as they are, decoded, for a tensor."},
    {"match_mask_batch", KW(mask<false, true>),
     "[extension] match_mask_batch(haystacks, overlapping=False, *, offsets=None, row_length=None) -> MaskedRows: "
     "match_mask of every row in one call: .data is 1 where a match covers the byte, else 0."},
    {"cover_spans", KW(spans<false>),
     "cover_spans(haystack, overlapping=False, *, gap=0) -> MatchSpans\n\n[extension] the union of the matches that "
     "find_matches_as_indexes(haystack, overlapping) reports, as two int64 columns .start / .end: matches that overlap, "
     "touch or lie at most gap positions apart are ONE span -- the ranges to highlight, cut or redact.  The spans are "
     "ascending and disjoint and next.start - prev.end > gap; with gap=0 they are the runs of ones of match_mask.  "
     "AhoCorasick: character indexes; BytesAhoCorasick: byte offsets, and a __dlpack__ tensor on the automaton's device is "
     "searched and merged there -- nothing but the number of spans crosses the bus.  gap: an int 0 .. 2**63 - 1."},
    {"cover_spans_batch", KW(spans<true>),
     "cover_spans_batch(haystacks, overlapping=False, *, gap=0, offsets=None, row_length=None) -> MatchSpans\n\n"
     "[extension] cover_spans of every row in one call, with .row_offsets: spans row_offsets[h] .. row_offsets[h + 1] - 1 "
     "are row h's, their offsets local to it; spans never join across rows.  haystacks: a sequence, or ONE 1-D contiguous "
     "uint8 __dlpack__ tensor cut by exactly one of offsets and row_length, as for count_by_pattern_sparse_batch (byte "
     "offsets for a tensor).  A tensor on the automaton's device is searched and merged there and the columns stay there."},
    {"find_matches_as_snippets", KW(snippets<false>),
     "find_matches_as_snippets(haystack, overlapping=False, *, context=0) -> MatchSnippets\n\n[extension] one snippet per "
     "match that find_matches_as_columns(haystack, overlapping) reports, in its order: the matched text and up to context "
     "BYTES on each side of it, clipped to the haystack, as the caller's own bytes (.data, cut by .offsets; the match begins "
     ".lead bytes into its snippet; .pattern is the columns' pattern).  AhoCorasick: UTF-8 bytes, the ends moved inward to a "
     "character boundary, so tolist() is a list[str] and with context=0 it equals find_matches_as_strings.  "
     "BytesAhoCorasick: a __dlpack__ tensor on the automaton's device is searched and cut there -- nothing but the size of "
     "the data crosses the bus.  context: an int 0 .. 2**63 - 1."},
    {"find_matches_as_snippets_batch", KW(snippets<true>),
     "find_matches_as_snippets_batch(haystacks, overlapping=False, *, context=0, offsets=None, row_length=None) -> "
     "MatchSnippets\n\n[extension] find_matches_as_snippets of every row in one call, with .row_offsets: snippets "
     "row_offsets[h] .. row_offsets[h + 1] - 1 are row h's; a snippet never crosses a row.  haystacks: a sequence, or ONE 1-D "
     "contiguous uint8 __dlpack__ tensor cut by exactly one of offsets and row_length, as for cover_spans_batch.  A tensor on "
     "the automaton's device is searched and cut there and every part stays there."},
    {"label_tokens", KW(label_tokens<false>),
     "label_tokens(haystack, token_offsets, overlapping=False) -> TokenLabels\n\n[extension] the matches that "
     "find_matches_as_indexes(haystack, overlapping) reports, mapped onto tokens: token t is haystack[token_offsets[t]:"
     "token_offsets[t + 1]], and a match touches it iff token_offsets[t] < end and token_offsets[t + 1] > start (an empty "
     "token strictly inside a match is touched, one on its edge is not).  .pattern[t] is the pattern of the FIRST touching "
     "match in the search's order, or -1; .begin[t] is 1 where that match's tokens begin (the B of BIO).  token_offsets: "
     "k + 1 boundaries that do not decrease, within 0 .. len(haystack) -- a sequence of ints or an int64 buffer; "
     "AhoCorasick: CHARACTER indexes, the unit of find_matches_as_indexes and of a tokenizer's offset_mapping; "
     "BytesAhoCorasick: byte offsets, and with a __dlpack__ tensor on the automaton's device as haystack, token_offsets is a "
     "1-D int64 __dlpack__ tensor there and the search and the labels stay in HBM."},
    {"label_tokens_batch", KW(label_tokens<true>),
     "label_tokens_batch(haystacks, token_offsets, overlapping=False, *, offsets=None, row_length=None) -> TokenLabels\n\n"
     "[extension] label_tokens over a batch in one call.  haystacks a sequence: token_offsets has one entry per haystack, "
     "each that haystack's local boundaries (characters for AhoCorasick, else bytes); a token never crosses a haystack, "
     ".row_offsets cuts the tokens by haystack and tolist() gives one list per haystack.  haystacks ONE 1-D contiguous uint8 "
     "__dlpack__ tensor cut by exactly one of offsets and row_length, as for mask_all_batch: token_offsets is ONE 1-D "
     "contiguous int64 __dlpack__ tensor of T + 1 GLOBAL byte boundaries on the same device, tokens may cross rows, and on "
     "the automaton's device everything stays in HBM.  There the boundaries are the caller's word, as offsets are: arrays "
     "that do not rise give wrong labels, never a write outside the T entries.  The call returns with the labels still being "
     "made: the TokenLabels keeps the three input tensors alive until it goes, and they must not be written before an accessor "
     "of a column has returned."},
    {"match_at", KW(match_at),
     "match_at(haystack, positions, overlapping=False, *, offsets=None, row_length=None) -> MatchesAt\n\n[extension] the "
     "crate's anchored search: for every position, the pattern that begins exactly there -- by the object's match kind: "
     "Standard the shortest (then the lowest index), LeftmostFirst the lowest index (re.match of the alternation), "
     "LeftmostLongest the longest -- as (pattern, end), or (-1, -1).  overlapping=True (Standard objects only): every such "
     "pattern, ordered by end, then by index, with .row_offsets cutting them by position.  No search runs: a few bytes are "
     "read per position.  positions: a sequence of ints or an int64 buffer within 0 .. len(haystack) (ValueError), any order, "
     "repeats allowed; AhoCorasick: CHARACTER indexes in and out.  BytesAhoCorasick with a uint8 __dlpack__ tensor: positions "
     "is ONE 1-D contiguous int64 __dlpack__ tensor of byte positions on the same device, and offsets / row_length cut the "
     "tensor into rows as for mask_all_batch (split_rows(t).offsets included): a match never crosses its position's row.  On "
     "the automaton's device everything stays in HBM; positions are then the caller's word -- one outside the data gives "
     "(-1, -1) -- and the MatchesAt keeps the input tensors alive until it goes: they must not be written before an accessor "
     "of a column has returned."},
    {"match_prefix_batch", KW(match_prefix_batch),
     "match_prefix_batch(haystacks, overlapping=False, *, full=False, offsets=None, row_length=None) -> MatchesAt\n\n"
     "[extension] match_at at the start of every row, in one call: one (pattern, end) per row, end being the length of the "
     "match (characters for AhoCorasick) -- prefix block lists, log levels, routing by key prefix.  full=True: only a pattern "
     "that IS the row counts -- a dictionary lookup, strings to ids; every match kind then reports the lowest index.  "
     "haystacks: a sequence, or ONE 1-D contiguous uint8 __dlpack__ tensor cut by exactly one of offsets and row_length, as "
     "for filter_batch.  A tensor on the automaton's device stays in HBM, and so does the result."},
    {"segment", KW(segment<false>),
     "segment(haystack, *, utf8=None) -> Segments\n\n[extension] greedy tokenization by the dictionary: the haystack cut into "
     "the object's patterns from left to right -- at every position the pattern the object's match kind prefers there (what "
     "match_at reports: LeftmostLongest the longest, which makes this MaxMatch, WordPiece's inner loop and forward maximum "
     "matching; LeftmostFirst the lowest index, re.finditer of P_0|P_1|...|.; Standard the shortest), going on where it ended.  "
     "Where no pattern begins the piece is an unknown unit with pattern -1: one byte, or with utf8=True one whole UTF-8 "
     "character (an ill-formed one: its lead byte and the continuation bytes that follow).  utf8=None: True for AhoCorasick, "
     "False for BytesAhoCorasick; anything but a bool or None: TypeError.  The pieces tile the haystack.  No search runs, and "
     "patterns longer than 256 bytes are refused (ValueError).  AhoCorasick: boundaries are CHARACTER indexes.  "
     "BytesAhoCorasick with a uint8 __dlpack__ tensor on the automaton's device: everything stays in HBM, and the Segments keeps "
     "the tensor alive until it goes: it must not be written before an accessor of a column has returned."},
    {"segment_batch", KW(segment<true>),
     "segment_batch(haystacks, *, utf8=None, offsets=None, row_length=None) -> Segments\n\n[extension] segment for every row in "
     "one call: a piece never crosses a row, .offsets holds the GLOBAL boundaries of all pieces -- exactly what "
     "label_tokens_batch takes as token_offsets for a tensor -- and .row_offsets cuts the pieces by row.  haystacks: a "
     "sequence, or ONE 1-D contiguous uint8 __dlpack__ tensor cut by exactly one of offsets and row_length, as for "
     "filter_batch (split_rows(t).offsets included).  A tensor on the automaton's device stays in HBM, and so does the result: "
     "split_rows -> segment_batch -> label_tokens_batch / filter_batch runs without anything leaving the device."},
    {"wordpiece", KW(wordpiece<false>),
     "wordpiece(haystack, *, continuation_prefix=\"##\", separators=None, isolated=None, max_word_bytes=100, unk_id=-1) -> "
     "WordPieces\n\n[extension] WordPiece tokenization by the dictionary, on the device.  The patterns are the vocabulary as a "
     "vocab.txt lists it: whole-word entries as they are, continuation entries with the prefix.  The haystack is cut into "
     "words -- a byte in separators (None: ASCII_WHITESPACE) belongs to no word, a byte in isolated (None: none; "
     "ASCII_PUNCTUATION is BertTokenizer's) is a word by itself, every other run of bytes is a word -- and every word into "
     "the entries the automaton's matchkind prefers, the first one looked up as it stands, the following ones behind the "
     "prefix.  A word longer than max_word_bytes, or one in which a step finds no entry, is ONE piece with unk_id.  With "
     "MatchKind.LeftmostLongest this is BERT's WordpieceTokenizer over text.split(), the word limit counted in bytes.  The "
     "ids are pattern indexes.  Both sets are bytes-like; for AhoCorasick they and the prefix may be str, the sets ASCII.  "
     "AhoCorasick: a str, positions in characters.  BytesAhoCorasick: a bytes-like, or a uint8 __dlpack__ tensor on the "
     "automaton's device: everything stays in HBM, and the WordPieces keeps the tensor alive."},
    {"wordpiece_batch", KW(wordpiece<true>),
     "wordpiece_batch(haystacks, *, continuation_prefix=\"##\", separators=None, isolated=None, max_word_bytes=100, unk_id=-1, "
     "offsets=None, row_length=None) -> WordPieces\n\n[extension] wordpiece for every row in one call: a word never crosses a "
     "row, .start and .end hold GLOBAL positions and .row_offsets cuts the pieces by row.  haystacks: a sequence, or ONE 1-D "
     "contiguous uint8 __dlpack__ tensor cut by exactly one of offsets and row_length, as for segment_batch "
     "(split_rows(t).offsets included).  A tensor on the automaton's device stays in HBM, and so does the result."},
    {"find_whole_words_as_columns", KW(whole_words<0>),
     "find_whole_words_as_columns(haystack, overlapping=False, *, matchkind=MatchKind.LeftmostLongest, word_bytes=None) -> "
     "MatchColumns\n\n[extension] grep -w for the object's patterns: of all their occurrences those whose neighbour bytes "
     "(the byte in front of the match and the byte behind it; a haystack's ends are boundaries) are no word bytes, and of "
     "those the non-overlapping ones matchkind picks (overlapping=True: all of them, in the overlapping search's order).  "
     "The object must be a MatchKind.Standard one (ValueError otherwise): the search behind it is an overlapping one, and "
     "matchkind resolves the whole-word occurrences only -- with ['he cat', 'cat'] on 'the cat' the result is cat at 4, "
     "which a filter over a leftmost search loses.  word_bytes: None (ASCII_WORD_BYTES: [0-9A-Za-z_]) or a bytes-like of the "
     "byte values that count as word bytes.  AhoCorasick: character indexes (the test runs on UTF-8 bytes); "
     "BytesAhoCorasick: byte offsets, and a __dlpack__ tensor on the automaton's device is searched, tested and resolved "
     "there."},
    {"find_whole_words_as_columns_batch", KW(whole_words<1>),
     "find_whole_words_as_columns_batch(haystacks, overlapping=False, *, matchkind=MatchKind.LeftmostLongest, "
     "word_bytes=None, offsets=None, row_length=None) -> MatchColumns\n\n[extension] find_whole_words_as_columns of every row "
     "in one call, with .row_offsets; a row's first byte is never the neighbour of the row before it.  haystacks: a sequence, "
     "or ONE 1-D contiguous uint8 __dlpack__ tensor cut by exactly one of offsets and row_length, as for "
     "count_by_pattern_sparse_batch (byte offsets local to the row for a tensor).  A tensor on the automaton's device is "
     "searched and resolved there and the columns stay there."},
    {"filter_whole_words_batch", KW(whole_words<2>),
     "filter_whole_words_batch(haystacks, overlapping=False, *, matchkind=MatchKind.LeftmostLongest, word_bytes=None, "
     "keep='unmatched', min_matches=1, offsets=None, row_length=None) -> FilteredRows\n\n[extension] filter_batch with a row's "
     "matches counted as find_whole_words_as_columns_batch reports them: a block list applied by whole word keeps 'class' "
     "and 'Scunthorpe'.  .data is the caller's own bytes."},
    {"find_matches_as_columns", KW(columns<false>),
     "[extension] find_matches_as_indexes(haystack, overlapping) as a MatchColumns: three int64 columns (pattern, start, "
     "end) exported through DLPack, in host memory for a host haystack and in HBM on the automaton's device for a "
     "__dlpack__ tensor there -- no tuple list, and for a tensor nothing but the number of matches crosses the bus.  The "
     "call returns once that number is known; every accessor of a column, __dlpack__ included, waits for the split kernel "
     "first, so a consumer on any stream sees finished data."},
    {"find_matches_as_columns_batch", KW(columns<true>),
     "[extension] find_matches_as_indexes_batch(haystacks, overlapping) as a MatchColumns with row_offsets: rows "
     "row_offsets[h] .. row_offsets[h + 1] are haystack h's matches, their offsets local to it."},
};

const PyMethodDef AC_METHODS[] = {
    {"find_matches_as_strings", KW(ac_find_strings),
     "Return matches as list of patterns (i.e. strings). If ``overlapping`` is ``False`` (the "
     "default), don't include overlapping results."},
    {"replace_all", KW(replace_all),
     "[extension] the haystack with every non-overlapping match (as find_matches_as_indexes reports them) replaced by "
     "replace_with[pattern index]; replace_with has one str per pattern (ValueError otherwise)."},
};
const PyMethodDef BAC_METHODS[] = {
    {"replace_all", KW(replace_all),
     "[extension] the haystack (a buffer, or a __dlpack__ tensor on the automaton's device) as bytes with every "
     "non-overlapping match replaced by replace_with[pattern index]; replace_with has one buffer per pattern."},
};
#undef KW

// One automaton class in the module: its own methods, then the shared ones.  The table lives as long as the type.
template <size_t N>
PyTypeObject *register_automaton_type(PyObject *module, const char *name, int size, newfunc tp_new, const char *doc, const PyMethodDef (&own)[N]) {
    std::vector<PyMethodDef> *methods = new std::vector<PyMethodDef>(own, own + N);
    methods->insert(methods->end(), std::begin(SHARED_METHODS), std::end(SHARED_METHODS));
    methods->push_back({nullptr, nullptr, 0, nullptr});
    PyType_Slot slots[] = {
        {Py_tp_new, reinterpret_cast<void *>(tp_new)},
        {Py_tp_dealloc, reinterpret_cast<void *>(automaton_dealloc)},
        {Py_tp_methods, methods->data()},
        {Py_tp_doc, const_cast<char *>(doc)},
        {0, nullptr},
    };
    PyType_Spec spec = {name, size, 0, Py_TPFLAGS_DEFAULT, slots};
    PyObject *tp = PyType_FromSpec(&spec);
    if (!tp || PyModule_AddObject(module, strchr(name, '.') + 1, tp) < 0) { Py_XDECREF(tp); return nullptr; }
    return reinterpret_cast<PyTypeObject *>(tp);
}

PyMethodDef module_methods[] = {
    {"split_rows", reinterpret_cast<PyCFunction>(reinterpret_cast<void (*)()>(mod_split_rows)), METH_VARARGS | METH_KEYWORDS,
     "[extension] split_rows(data, delimiter=b'\\n') -> RowOffsets: the offsets that cut a delimited buffer into rows -- 0, "
     "then p + 1 for every byte p that equals the delimiter, then len(data) if the last byte is not one.  The delimiter ends "
     "its row (splitlines(keepends=True) for '\\n'), no row is empty.  data: one 1-D contiguous uint8 __dlpack__ tensor -- on a "
     "ROCm device it is cut where it lies and the offsets stay there -- or any contiguous byte buffer; it is never written.  "
     "delimiter: an int in range(256), a one-byte buffer or a one-character ASCII str.  Pass the result's .offsets as "
     "offsets= to the _batch methods that take a tensor."},
    {"_mask_fill", mod_mask_fill, METH_VARARGS,
     "_mask_fill(fill, text) -> int: the fill byte mask_all takes from `fill` (text: the str class's rule), or its error"},
    {"_spans_gap", mod_spans_gap, METH_O,
     "_spans_gap(gap) -> int: the gap cover_spans takes from its `gap` argument, or its error"},
    {"_wordpiece_args", mod_wordpiece_args, METH_VARARGS,
     "_wordpiece_args(str_class, continuation_prefix=None, separators=None, isolated=None, max_word_bytes=None, unk_id=None) -> "
     "(cls, prefix, max_word_bytes, unk_id): what wordpiece takes from its keyword arguments -- the 256 byte classes (0 word, "
     "1 separator, 2 isolated), the prefix's bytes and the two ints -- or their error"},
    {"_snippets_context", mod_snippets_context, METH_O,
     "_snippets_context(context) -> int: the budget find_matches_as_snippets takes from its `context` argument, or its error"},
    {"_mask_per_character", mod_mask_per_character, METH_VARARGS,
     "_mask_per_character(haystack, row, text) -> str | bytes: a str haystack's masked row (one entry per UTF-8 byte) as "
     "mask_all (text) / match_mask return it: one entry per character"},
    {nullptr, nullptr, 0, nullptr},
};

PyModuleDef moduledef = {
    PyModuleDef_HEAD_INIT, "ahocorasick_rs",
    "MI355X-native Aho-Corasick matcher behind the ahocorasick_rs API (HIP kernels via libacx_hip.so).",
    -1, module_methods, nullptr, nullptr, nullptr, nullptr,
};

} // namespace

extern "C" __attribute__((visibility("default"))) PyObject *PyInit_ahocorasick_rs(void) {
    PyObject *m = PyModule_Create(&moduledef);
    if (!m) return nullptr;
    static const char *mk_v[] = {"Standard", "LeftmostFirst", "LeftmostLongest"};
    static const char *mk_q[] = {"MatchKind.Standard", "MatchKind.LeftmostFirst",
                                 "MatchKind.LeftmostLongest"};
    static const char *im_v[] = {"NoncontiguousNFA", "ContiguousNFA", "DFA"};
    static const char *im_q[] = {"Implementation.NoncontiguousNFA", "Implementation.ContiguousNFA",
                                 "Implementation.DFA"};
    MatchKindType = make_enum(m, "MatchKind", "ahocorasick_rs.MatchKind", mk_v, mk_q, 3);
    ImplementationType = make_enum(m, "Implementation", "ahocorasick_rs.Implementation", im_v, im_q, 3);
    if (!MatchKindType || !ImplementationType) { Py_DECREF(m); return nullptr; }
    PyType_Spec col_spec = {"ahocorasick_rs.Column", sizeof(ColumnObject), 0,
                            Py_TPFLAGS_DEFAULT | Py_TPFLAGS_DISALLOW_INSTANTIATION, col_slots};
    ColumnType = reinterpret_cast<PyTypeObject *>(PyType_FromSpec(&col_spec));
    bool ok = ColumnType != nullptr;
    if (ok) Py_INCREF(ColumnType); // (the module holds one reference, the global the other)
    ok = ok && PyModule_AddObject(m, "Column", reinterpret_cast<PyObject *>(ColumnType)) == 0;
    for (ResultType &t : RESULT_TYPES) ok = ok && register_result_type(m, &t);
    AhoCorasickType = !ok ? nullptr : register_automaton_type(
        m, "ahocorasick_rs.AhoCorasick", sizeof(AcObject), ac_new,
        "Search for multiple pattern strings against a single haystack string.\n\n"
        "AhoCorasick(patterns, matchkind=MatchKind.Standard, store_patterns=None, implementation=None, "
        "ascii_case_insensitive=False)", AC_METHODS);
    ok = AhoCorasickType && register_automaton_type(
        m, "ahocorasick_rs.BytesAhoCorasick", sizeof(BacObject), bac_new,
        "Search for multiple pattern bytes against a single bytes haystack.\n\n"
        "BytesAhoCorasick(patterns, matchkind=MatchKind.Standard, implementation=None, ascii_case_insensitive=False)", BAC_METHODS);
    ok = ok && PyModule_AddObject(m, "ASCII_WORD_BYTES", PyBytes_FromString(ASCII_WORD_BYTES)) == 0;
    ok = ok && PyModule_AddObject(m, "ASCII_WHITESPACE", PyBytes_FromString(ASCII_WHITESPACE)) == 0;
    ok = ok && PyModule_AddObject(m, "ASCII_PUNCTUATION", PyBytes_FromString(ASCII_PUNCTUATION)) == 0;
    if (!ok) { Py_DECREF(m); return nullptr; }
    return m;
}
