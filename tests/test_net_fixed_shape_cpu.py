"""The fixed-shape form of the row-Winograd net kernel without a GPU: its code object ("Two forms of
the row-Winograd net kernel") and the interface around it."""
import os
import re

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def test_fixed_shape_kernel_keeps_two_waves_per_simd_and_no_scratch():
    """k_net_forward_w_c4 exists once, spills nothing (vector or scalar), has no scratch and at most 256 VGPRs: two
    waves per SIMD, as the general kernel -- tests/test_cpu_product.py's rule for the hot kernels; the general kernel and
    its run-time-depth twin keep their names (the tests that find them by name go on finding exactly them)"""
    from tests.test_cpu_product import _code_object_metadata
    md = _code_object_metadata("caro_net.hip.o")
    fixed = {n: k for n, k in md.items() if "k_net_forward_w_c4E" in n}
    assert len(fixed) == 1, sorted(md)
    (name, k), = fixed.items()
    assert k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0 and k[".vgpr_count"] <= 256, (name, k)
    assert k[".private_segment_fixed_size"] == 0, name
    assert k[".group_segment_fixed_size"] == 160 * 1024  # the LDS layout of the general kernel
    for other in ("k_net_forward_wE", "k_net_forward_w_anyE"):
        assert sum(other in n for n in md) == 1, other
    general = next(k for n, k in md.items() if "k_net_forward_wE" in n)
    assert k[".kernarg_segment_size"] < general[".kernarg_segment_size"]  # one parameter block, no row1


def test_the_form_switch_is_declared_bound_and_checks_its_arguments():
    """the three calls are in the header, the binding and the library; without a net handle they refuse (host only)"""
    from caro_ai_amd import _lib
    L = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "caro_hip.h")).read()
    for name in ("caro_net_set_kernel_form", "caro_net_kernel_form", "caro_net_last_launch_form"):
        assert re.search(r"\b%s\(" % name, hdr) and name in _lib.EXPORTS and hasattr(L, name)
    assert L.caro_net_set_kernel_form(None, 0) < 0 and L.caro_last_error()
    assert L.caro_net_kernel_form(None) < 0 and L.caro_net_last_launch_form(None) < 0


def test_the_kernel_text_asks_the_trait_for_the_shape():
    """one source for both forms: inside the row-Winograd kernel and the functions it calls, no board quantity is read
    from the parameter block except as the argument of its accessor"""
    csrc = os.path.join(ROOT, "caro_ai_amd", "csrc")
    inc = open(os.path.join(csrc, "caro_net_kernels.inc")).read()
    body = inc[inc.index("#if CARO_ONE_NET\n__global__"):inc.index("/*@HST_PUBLISH")]
    hip = open(os.path.join(csrc, "caro_net.hip")).read()

    def fn(start, end):
        a = hip.index(start)
        return hip[a:hip.index(end, a)]

    texts = {"k_net_forward_w": body,
             "conv_in_mfma": fn("template <class S, bool K2D = false, int NTH = NT>\n__device__ __forceinline__ void conv_in_mfma", "\n}\n"),
             "trunk_w": fn("template <int KS, int NR, class S>", "#undef CARO_ALOAD"),
             "heads_f32 (what the row-Winograd kernels run)": fn("template <class S, bool STAGED", "  if (featbuf) {")}
    field = re.compile(r"\bp0?\.(H|W|HW|A|TB|TB2|TB4)\b")
    for what, text in texts.items():
        code = "\n".join(ln.split("//")[0] for ln in text.splitlines())
        for m in field.finditer(code):
            before = code[:m.start()]
            assert before.endswith("S::%s(" % m.group(1)), (what, code[max(0, m.start() - 60):m.end() + 20])
