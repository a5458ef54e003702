"""The chunked sums the backward passes share (csrc/grad_sums.hip), without a GPU: the file defines exactly the kernels
k_grad_tn and k_grad_reduce, the code object holds both, and the GPU case lists hold networks that launch them -- the
reduce from all three families, the dW kernel from the IDR backward (the texture and the SIREN backward keep dW kernels
of their own, guarded in their own files).  A new kernel of that file without a case fails here, on the CPU."""
import os
import re

from conftest import ROOT
from test_idr_backward_gpu import FORMS as IDR_FORMS, VALUE_ONLY as IDR_VALUE_ONLY
from test_siren_backward_gpu import BACKWARD_CASES as SIREN_CASES
from test_texture_backward_gpu import BACKWARD_CASES as TEXTURE_CASES

KERNELS = {"k_grad_tn", "k_grad_reduce"}


def test_gpu_cases_reach_every_grad_sums_kernel_of_the_library():
    from iso_points_amd import _lib
    from test_abi import _code_object_kernels
    src = open(os.path.join(ROOT, "iso_points_amd", "csrc", "grad_sums.hip")).read()
    defined = set(re.findall(r"__global__[^;{]*?\bvoid\s+(\w+)\s*\(", src))
    assert defined == KERNELS, "kernels of grad_sums.hip without a GPU case named here: %s" % sorted(defined ^ KERNELS)
    in_library = set()
    for name in (k[0] for k in _code_object_kernels()):
        m = re.search(r"_GLOBAL__N_1(\d+)(k_grad_\w*)", name)
        if m and m.group(2)[:int(m.group(1))] in KERNELS:
            # the rest of the mangled name is the parameter list: a template instance would begin with I
            assert not m.group(2)[int(m.group(1)):].startswith("I"), name
            in_library.add(m.group(2)[:int(m.group(1))])
    assert in_library == KERNELS, sorted(in_library)
    lib = _lib.load()
    # k_grad_reduce: the three lists are not empty and hold shapes the entries run
    assert TEXTURE_CASES and all(lib.iso_texgrad_form(*s) >= 0 for s in TEXTURE_CASES)
    assert SIREN_CASES and all(lib.iso_sirengrad_form(H, L) >= 800 for H, L, tan in SIREN_CASES)
    # k_grad_tn: every IDR network has two layers at least, so each has a dW_l, with and without the tangent rows
    for cases in (IDR_FORMS, IDR_VALUE_ONLY):
        assert cases and all(lib.iso_idrgrad_form(H, nl, -1 if skip is None else skip, nf) == 900 + H // 16 and nl >= 2
                             for H, nl, skip, nf in cases)
