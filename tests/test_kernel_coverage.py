"""CPU guard of the GPU suite's reach: every kernel entry point of include/tg_kernels.h (name ending in _f32 / _bf16) is called BY NAME
(a quoted name handed to lib.call, or an attribute call on the loaded library) from at least one tests/test_gpu_*.py, so that a kernel
added without a direct test fails here, on a machine without a GPU.

Layer and network tests do not count as a direct test: they run at the network's shapes and compare at network tolerances, which
cannot see a wrong tail column, garbage in the channel padding or a write past the end of an output.  The few exceptions are listed in
RUNTIME_NAMED (kernels whose tests build the entry point's name at run time, 'tg_igemm_' + prec) with the test that calls them, and
that test must exist and spell the name's prefix; in NOT_KERNELS (host functions named like kernels); and in THROUGH_WRAPPER (kernels
tested so far only through the package function that calls them, with that test).  Non-kernel symbols (descriptor builders, profiler,
graph capture, ...) do not end in _f32 / _bf16 and are outside the rule."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")

KERNEL_SUFFIXES = ("_f32", "_bf16")

# entry point -> (test that calls it, the literal prefix that test joins with the precision suffix, reason)
RUNTIME_NAMED = {
    "tg_igemm_multi_f32": ("test_gpu_igemm.py::test_cut_long_parities_of_a_transposed_conv_launch", "'tg_igemm_multi_' + prec",
                           "f32 / bf16 parametrised; name built from the precision"),
    "tg_igemm_multi_bf16": ("test_gpu_igemm.py::test_cut_long_parities_of_a_transposed_conv_launch", "'tg_igemm_multi_' + prec",
                            "f32 / bf16 parametrised; name built from the precision"),
    "tg_igemm_labels_f32": ("test_gpu_igemm.py::test_conv_writes_the_cond_concat_behind_it", '"tg_igemm_labels_" + prec',
                            "f32 / bf16 parametrised; name built from the precision"),
    "tg_igemm_labels_bf16": ("test_gpu_igemm.py::test_conv_writes_the_cond_concat_behind_it", '"tg_igemm_labels_" + prec',
                             "f32 / bf16 parametrised; name built from the precision"),
}

# host functions whose names end like a kernel's but launch nothing
NOT_KERNELS = {
    "tg_wgrad_splits_bf16": "host query: the pixel splits tg_wgrad_bf16 takes (no device work)",
}

# kernels whose only GPU test calls them through the package function that owns the call, held there to a float64 restatement:
# entry point -> (test, package file that calls the entry point by name, reason).  Each is a candidate for a direct per-kernel test.
# Empty: every kernel entry point has a direct test.
THROUGH_WRAPPER = {}
PKG = os.path.join(ROOT, "tensorflow-implementation-of-triple-gan_amd")


def _kernels():
    from tg import lib
    return sorted(n for n in lib.parse_header() if n.endswith(KERNEL_SUFFIXES))


def _gpu_test_sources():
    return {os.path.basename(p): open(p).read() for p in sorted(glob.glob(os.path.join(TESTS, "test_gpu_*.py")))}


def _called(name, text):
    """a call by name: the quoted string lib.call / lib.call_igemm take, or an attribute call on the loaded library (a mention in a
    docstring or comment does not count)."""
    n = re.escape(name)
    return re.search(r"(['\"])%s\1|\.%s\(" % (n, n), text) is not None


def test_every_kernel_entry_point_has_a_direct_gpu_test():
    srcs = _gpu_test_sources()
    everything = "\n".join(srcs.values())
    kernels = _kernels()
    assert len(kernels) >= 80
    listed = set(RUNTIME_NAMED) | set(NOT_KERNELS) | set(THROUGH_WRAPPER)
    missing = [n for n in kernels if n not in listed and not _called(n, everything)]
    assert not missing, "kernel entry points without a direct call in tests/test_gpu_*.py: %s" % ", ".join(missing)


def _test_body(srcs, test_id):
    fname, func = test_id.split("::")
    assert fname in srcs, test_id
    m = re.search(r"^def %s\(.*?(?=^def |\Z)" % re.escape(func), srcs[fname], flags=re.S | re.M)
    assert m, "%s names a test that does not exist" % test_id
    return m.group(0)


def test_other_allow_lists_are_current():
    """NOT_KERNELS / THROUGH_WRAPPER name declared symbols that no GPU test calls directly yet (an entry that gains a direct test must
    leave the list), and the wrapper named for each still calls it."""
    from tg import lib
    sigs = lib.parse_header()
    srcs = _gpu_test_sources()
    everything = "\n".join(srcs.values())
    assert not set(NOT_KERNELS) & set(THROUGH_WRAPPER) and not (set(NOT_KERNELS) | set(THROUGH_WRAPPER)) & set(RUNTIME_NAMED)
    for name, reason in NOT_KERNELS.items():
        assert name in sigs and reason, name
        assert not _called(name, everything), "%s is now called by name: drop it from NOT_KERNELS" % name
    for name, (test_id, pkg_file, reason) in THROUGH_WRAPPER.items():
        assert name in sigs and reason, "allow-listed %s is no longer declared in include/tg_kernels.h" % name
        assert not _called(name, everything), "%s is now called by name: drop it from THROUGH_WRAPPER" % name
        _test_body(srcs, test_id)
        assert _called(name, open(os.path.join(PKG, pkg_file)).read()), "%s no longer calls %s" % (pkg_file, name)


def test_runtime_named_allow_list_is_current():
    """every allow-listed name is still a kernel of the header, is not also called literally (the entry would be dead), and the test
    it names exists and builds the name from the listed prefix."""
    from tg import lib
    sigs = lib.parse_header()
    srcs = _gpu_test_sources()
    everything = "\n".join(srcs.values())
    for name, (test_id, prefix, reason) in RUNTIME_NAMED.items():
        assert name in sigs and name.endswith(KERNEL_SUFFIXES), "allow-listed %s is no longer declared in include/tg_kernels.h" % name
        assert reason
        assert not _called(name, everything), "%s is now called by name: drop it from RUNTIME_NAMED" % name
        assert prefix in _test_body(srcs, test_id), "%s does not build %s from %s" % (test_id, name, prefix)
        assert name.startswith(prefix.strip("'\"").split("'")[0].split('"')[0])
