"""ctypes binding of libblurrily_hip.so (include/blurrily_storage.h).

Fails loudly when the library is missing: there is no pure-Python or CPU path.
"""
import ctypes as C
import importlib.util
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
# BLURRILY_LIB selects another build of the same library (same-box A/B of two builds, tools/ab_probe.py)
LIB_PATH = os.environ.get("BLURRILY_LIB") or os.path.join(_HERE, "libblurrily_hip.so")


class TrigramMatch(C.Structure):
    """storage.h:18-24 -- packed 12-byte row."""
    _pack_ = 1
    _fields_ = [("reference", C.c_uint32), ("matches", C.c_uint32), ("weight", C.c_uint32)]


class TrigramStat(C.Structure):
    """storage.h:26-30."""
    _fields_ = [("references", C.c_uint32), ("trigrams", C.c_uint32)]


class DeviceInfo(C.Structure):
    _fields_ = [
        ("device_ordinal", C.c_int32), ("n_refs", C.c_uint32), ("n_windows", C.c_uint32),
        ("window_bits", C.c_uint32), ("n_entries", C.c_uint64), ("device_bytes", C.c_uint64),
        ("last_find_kernel_ms", C.c_double), ("last_tokenise_kernel_ms", C.c_double),
        ("n_pending", C.c_uint32), ("n_tombstones", C.c_uint32), ("base_builds", C.c_uint64),
        ("mean_hit_slice", C.c_double), ("n_bitmaps", C.c_uint32), ("reserved_", C.c_uint32),
        ("dense_share", C.c_double), ("ws_gain", C.c_double),
        ("n_replicas", C.c_uint32), ("distinct_devices", C.c_uint32), ("peer_access_mask", C.c_uint32),
        ("same_device_mask", C.c_uint32), ("pci_bus_id", C.c_char * 16),
    ]


_vp, _vpp = C.c_void_p, C.POINTER(C.c_void_p)
# every entry point of include/blurrily_storage.h: name -> (restype, argtypes)
_ENTRIES = {
    "blurrily_storage_new": (C.c_int, [_vpp]),
    "blurrily_storage_load": (C.c_int, [_vpp, C.c_char_p]),
    "blurrily_storage_close": (C.c_int, [_vpp]),
    "blurrily_storage_mark": (None, [_vp]),
    "blurrily_storage_save": (C.c_int, [_vp, C.c_char_p]),
    "blurrily_storage_put": (C.c_int, [_vp, C.c_char_p, C.c_uint32, C.c_uint32]),
    "blurrily_storage_delete": (C.c_int, [_vp, C.c_uint32]),
    "blurrily_storage_find": (C.c_int, [_vp, C.c_char_p, C.c_uint16, C.c_void_p]),
    "blurrily_storage_stats": (C.c_int, [_vp, C.POINTER(TrigramStat)]),
    "blurrily_storage_put_many": (C.c_long, [_vp, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "blurrily_storage_find_batch": (C.c_int, [_vp, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint16,
                                              C.c_void_p, C.c_void_p]),
    "blurrily_storage_find_batch_device": (C.c_int, [_vp, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                                     C.c_uint16, C.c_void_p, C.c_void_p, C.c_void_p,
                                                     C.c_void_p]),
    "blurrily_storage_find_batch_raw": (C.c_int, [_vp, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint16,
                                                  C.c_void_p, C.c_void_p, C.c_void_p]),
    "blurrily_normalize_batch_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                                  C.c_void_p]),
    "blurrily_storage_sync_device": (C.c_int, [_vp]),
    "blurrily_tokeniser_parse_string": (C.c_int, [C.c_char_p, C.c_void_p]),
    "blurrily_storage_device_info": (C.c_int, [_vp, C.POINTER(DeviceInfo)]),
    "blurrily_storage_set_timing": (None, [_vp, C.c_int]),
    "blurrily_storage_set_stats": (None, [_vp, C.c_int]),
    "blurrily_storage_find_stats": (C.c_int, [_vp, C.c_void_p]),
    "blurrily_storage_set_option": (C.c_int, [_vp, C.c_char_p, C.c_longlong]),
    "blurrily_storage_get_option": (C.c_int, [_vp, C.c_char_p, C.POINTER(C.c_longlong)]),
    "blurrily_storage_find_path_flags": (C.c_int, [_vp, C.c_void_p, C.c_size_t]),
    "blurrily_storage_device_info_sized": (C.c_size_t, [_vp, C.c_void_p, C.c_size_t]),
    "blurrily_storage_tune": (C.c_int, [_vp, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_uint16]),
    "blurrily_storage_last_kernels": (C.c_size_t, [_vp, C.c_char_p, C.c_size_t]),
    # by reference (reference storage.h:72-87's commented-out get, and find by a stored reference)
    "blurrily_storage_get": (C.c_int, [_vp, C.c_uint32, C.c_void_p, C.c_int, C.c_void_p]),
    "blurrily_storage_get_batch": (C.c_int, [_vp, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_size_t]),
    "blurrily_storage_find_references": (C.c_int, [_vp, C.c_void_p, C.c_size_t, C.c_uint16, C.c_void_p, C.c_void_p,
                                                   C.c_void_p]),
    "blurrily_storage_find_references_device": (C.c_int, [_vp, C.c_void_p, C.c_size_t, C.c_uint16, C.c_void_p,
                                                          C.c_void_p, C.c_void_p, C.c_void_p]),
    # scoped find: a fixed set of references, and finds among them only
    "blurrily_scope_new": (C.c_int, [_vp, C.c_void_p, C.c_size_t, _vpp]),
    "blurrily_scope_close": (C.c_int, [_vpp]),
    "blurrily_scope_members": (C.c_int, [_vp, C.POINTER(C.c_uint32)]),
    "blurrily_storage_find_in": (C.c_int, [_vp, _vp, C.c_char_p, C.c_uint16, C.c_void_p]),
    "blurrily_storage_find_batch_in": (C.c_int, [_vp, _vp, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint16,
                                                 C.c_void_p, C.c_void_p]),
    "blurrily_storage_find_batch_in_device": (C.c_int, [_vp, _vp, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                                        C.c_uint16, C.c_void_p, C.c_void_p, C.c_void_p]),
    # a scope per needle: batched scoped find and find-by-reference, each needle among its own scope
    "blurrily_storage_find_batch_each_in": (C.c_int, [_vp, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                                      C.c_void_p, C.c_size_t, C.c_uint16, C.c_void_p, C.c_void_p]),
    "blurrily_storage_find_batch_each_in_device": (C.c_int, [_vp, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                                             C.c_size_t, C.c_void_p, C.c_size_t, C.c_uint16,
                                                             C.c_void_p, C.c_void_p, C.c_void_p]),
    "blurrily_storage_find_references_each_in": (C.c_int, [_vp, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                                           C.c_size_t, C.c_uint16, C.c_void_p, C.c_void_p,
                                                           C.c_void_p]),
    # threshold find: every row at or above a bar of matches
    "blurrily_storage_find_batch_above": (C.c_int, [_vp, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32,
                                                    C.c_void_p, C.c_uint64, C.c_void_p]),
    "blurrily_storage_find_above": (C.c_int, [_vp, C.c_char_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64,
                                              C.POINTER(C.c_uint64)]),
    "blurrily_storage_find_references_above": (C.c_int, [_vp, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32,
                                                         C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    # similarity find: the best rows by trigram Jaccard similarity
    "blurrily_storage_find_batch_similar": (C.c_int, [_vp, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint16,
                                                      C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "blurrily_storage_find_similar": (C.c_int, [_vp, C.c_char_p, C.c_uint16, C.c_uint32, C.c_void_p, C.c_void_p]),
    "blurrily_storage_find_references_similar": (C.c_int, [_vp, C.c_void_p, C.c_size_t, C.c_uint16, C.c_uint32,
                                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    # scoped similarity find: the similarity find among a scope's members, one scope or a scope per needle
    "blurrily_storage_find_batch_similar_in": (C.c_int, [_vp, _vp, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint16,
                                                         C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "blurrily_storage_find_similar_in": (C.c_int, [_vp, _vp, C.c_char_p, C.c_uint16, C.c_uint32, C.c_void_p,
                                                   C.c_void_p]),
    "blurrily_storage_find_batch_similar_each_in": (C.c_int, [_vp, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                                              C.c_void_p, C.c_size_t, C.c_uint16, C.c_uint32,
                                                              C.c_void_p, C.c_void_p, C.c_void_p]),
    "blurrily_storage_find_references_similar_each_in": (C.c_int, [_vp, C.c_void_p, C.c_size_t, C.c_void_p,
                                                                   C.c_void_p, C.c_size_t, C.c_uint16, C.c_uint32,
                                                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    # scoped threshold find: the threshold find among a scope's members, one scope or a scope per needle
    "blurrily_storage_find_batch_above_in": (C.c_int, [_vp, _vp, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32,
                                                       C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p]),
    "blurrily_storage_find_above_in": (C.c_int, [_vp, _vp, C.c_char_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64,
                                                 C.POINTER(C.c_uint64)]),
    "blurrily_storage_find_batch_above_each_in": (C.c_int, [_vp, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                                            C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32,
                                                            C.c_void_p, C.c_uint64, C.c_void_p]),
    "blurrily_storage_find_references_above_each_in": (C.c_int, [_vp, C.c_void_p, C.c_size_t, C.c_void_p,
                                                                 C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32,
                                                                 C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    # clusters: connected components of the similarity self-join, one label per reference
    "blurrily_storage_cluster": (C.c_int, [_vp, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p,
                                           C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]),
    # ... at several floors from one sweep: labels, components and edges per floor
    "blurrily_storage_cluster_levels": (C.c_int, [_vp, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32, C.c_void_p,
                                                  C.c_void_p, C.c_void_p]),
    # ... with each node's degree, each component's centre and whether a node shares an edge with its centre
    "blurrily_storage_cluster_centres": (C.c_int, [_vp, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p, C.c_void_p,
                                                   C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32),
                                                   C.POINTER(C.c_uint64)]),
    # density-based clusters over the same edges: cores, borders and noise
    "blurrily_storage_cluster_cores": (C.c_int, [_vp, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_void_p,
                                                 C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64),
                                                 C.POINTER(C.c_uint64)]),
    # the clusters of old and new references together, from the old ones' labels and a sweep of the new ones alone
    "blurrily_storage_cluster_extend": (C.c_int, [_vp, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                                  C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32),
                                                  C.POINTER(C.c_uint64)]),
    # clusters within caller-given blocks: an edge needs both ends under one block key
    "blurrily_storage_cluster_within": (C.c_int, [_vp, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p,
                                                  C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]),
    # the single-linkage dendrogram: the maximum spanning forest of the edges, heights in whole per mille
    "blurrily_storage_cluster_tree": (C.c_int, [_vp, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p, C.c_void_p,
                                                C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]),
    # ... of old and new references together, from the old ones' records and sweeps of the new ones alone
    "blurrily_storage_cluster_tree_extend": (C.c_int, [_vp, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p,
                                                       C.c_size_t, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                                       C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                                       C.POINTER(C.c_uint64)]),
    # the dendrogram of cluster_cores' cores: core heights, and the forest of the edges capped by them
    "blurrily_storage_cluster_core_tree": (C.c_int, [_vp, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_void_p,
                                                     C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32),
                                                     C.POINTER(C.c_uint32), C.POINTER(C.c_uint64),
                                                     C.POINTER(C.c_uint64)]),
    # the dendrogram within caller-given blocks: the forest of the edges whose ends carry one block key
    "blurrily_storage_cluster_tree_within": (C.c_int, [_vp, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p,
                                                       C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                                       C.POINTER(C.c_uint64)]),
    # the edges themselves, each pair once, as sorted {a, b, permille} records: capacity protocol, n_edges required
    "blurrily_storage_cluster_edges": (C.c_int, [_vp, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p, C.c_uint64,
                                                 C.POINTER(C.c_uint64)]),
    # ... of the graph within caller-given blocks
    "blurrily_storage_cluster_edges_within": (C.c_int, [_vp, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32,
                                                        C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]),
    # ... over two lists: only the edges with a new end (the second list's), from a sweep of the new ones alone
    "blurrily_storage_cluster_edges_extend": (C.c_int, [_vp, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_uint32,
                                                        C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]),
    # ... only the edges with one end in each list (record linkage), from a sweep of the smaller side
    "blurrily_storage_cluster_edges_between": (C.c_int, [_vp, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_uint32,
                                                         C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]),
    # cluster_cores within caller-given blocks: a degree counts the edges whose ends carry one block key
    "blurrily_storage_cluster_cores_within": (C.c_int, [_vp, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32,
                                                        C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32),
                                                        C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    # the core tree within caller-given blocks: core heights and the forest over the edges under one block key
    "blurrily_storage_cluster_core_tree_within": (C.c_int, [_vp, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32,
                                                            C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                                            C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                                            C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    # cluster extend within blocks: old labels as seeds, only the new references looked at, inside one block key
    "blurrily_storage_cluster_extend_within": (C.c_int, [_vp, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                                         C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p,
                                                         C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]),
}
EXPORTED_SYMBOLS = tuple(_ENTRIES)

_lib = None


def _one_hip_runtime():
    """A process must run on ONE copy of the HIP runtime.  PyTorch-ROCm ships its own
    libamdhip64.so.7 and loads it by path; if this library came first, bound to /opt/rocm's copy,
    the two runtimes would not see each other's streams and device pointers (torch tensors handed to
    blurrily_storage_find_batch_device, as bench.py does).  The dynamic linker resolves our
    DT_NEEDED by soname against what is already loaded, so: when torch is installed but not yet
    imported, load its copy first -- whichever order the application imports things in, everybody
    then shares it.  torch itself is not imported."""
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        return
    if spec is None or not spec.origin:
        return
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def hip_runtime():
    """ctypes handle of the HIP runtime the library is bound to (tests allocate through it)."""
    lib()
    return C.CDLL("libamdhip64.so.7")


def lib():
    """Load the shared library once; raise if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  blurrily_amd has no CPU fallback.")
    _one_hip_runtime()
    L = C.CDLL(LIB_PATH, use_errno=True)
    for name, (res, args) in _ENTRIES.items():
        try:
            fn = getattr(L, name)
        except AttributeError:
            if os.environ.get("BLURRILY_LIB"):      # (an older build of the library under A/B: it lacks the newer entry points)
                continue
            raise
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


NO_SCOPE = 0xFFFFFFFF                                  # BLURRILY_NO_SCOPE: a needle of such a batch with no scope
NO_CLUSTER = 0xFFFFFFFF                                # BLURRILY_NO_CLUSTER: the label of a reference the map does not hold
KIND_NONE, KIND_NOISE, KIND_BORDER, KIND_CORE = 0, 1, 2, 3   # BLURRILY_KIND_*: the kinds of a cluster_cores call
CLUSTER_MAX_LEVELS = 8                                 # BLURRILY_CLUSTER_MAX_LEVELS: the floors one cluster_levels call takes
NO_CORE = 0xFFFFFFFF                                   # BLURRILY_NO_CORE: the core height of a reference that has none
CLUSTER_TREE_MAX = 1 << 27                             # BLURRILY_CLUSTER_TREE_MAX: the references one cluster_tree call takes
