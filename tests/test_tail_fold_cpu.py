"""include/resdepth_hip_tail.h without a GPU: the side header against _lib.SIGNATURES_TAIL and the library's exports, its place in
the main header and in the build, and the two names living in that header and that table alone (tests/test_host_cpu.py and the
ledger of tests/test_memory_contract_gpu.py pin the main header's set)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"rd_bn_act_pool_fwd_tailskip", "rd_conv3x3_last_fwd_tail_pre"}


def _side_header():
    text = open(os.path.join(ROOT, "include", "resdepth_hip_tail.h")).read()
    return text, re.sub(r"/\*.*?\*/", " ", text, flags=re.S)


def test_side_header_signatures_and_exports():
    from resdepth_amd import _lib
    text, code = _side_header()
    exported = set(re.findall(r"\b(rd_\w+)\s*\(", code))
    assert exported == set(_lib.SIGNATURES_TAIL) == NAMES
    for name, (_, args) in _lib.SIGNATURES_TAIL.items():
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, code).group(1)
        assert len(decl.split(",")) == len(args), name
    lib = _lib.load()
    for name in NAMES:
        assert hasattr(lib, name), name
    # the header owns up to what is asked of it: the memory contract and the reference lines
    flat = re.sub(r"\s*\n \*\s*", " ", text)
    for phrase in ("lib/UNet.py:45,29-31,161", "lib/UNet.py:227-244", "Memory: reads", "and nothing else", "No scratch",
                   "bn_act_pool_tailskip_kernel", "conv_last_fwd_pre_kernel", "the first maximum wins"):
        assert phrase in flat, phrase


def test_the_header_is_included_from_the_main_header_and_named_in_the_build():
    main = open(os.path.join(ROOT, "include", "resdepth_hip.h")).read()
    assert main.count('#include "resdepth_hip_tail.h"') == 1
    for name in NAMES:
        assert name not in re.sub(r'#include "resdepth_hip_tail.h".*', "", main), name
    assert "resdepth_hip_tail.h" in open(os.path.join(ROOT, "resdepth_amd", "csrc", "build.sh")).read()
    csrc = os.path.join(ROOT, "resdepth_amd", "csrc")
    src = open(os.path.join(csrc, "rd_edge_conv.hip")).read()
    for kernel in ("bn_act_pool_tailskip_kernel<8>", "bn_act_pool_tailskip_kernel<4>", "bn_act_pool_tailskip_kernel<2>",
                   "conv_last_fwd_pre_kernel"):
        assert re.search(r"RD_LAUNCH\(%s," % re.escape(kernel), src), kernel       # the launch plan records them


def test_the_names_live_in_this_header_and_this_table_alone():
    from resdepth_amd import _lib
    inc = os.path.join(ROOT, "include")
    for other in sorted(os.listdir(inc)):
        if other != "resdepth_hip_tail.h":
            body = open(os.path.join(inc, other)).read()
            for name in NAMES:
                assert name not in body, (other, name)
    tables = [t for t in dir(_lib) if t.startswith("SIGNATURES") and t != "SIGNATURES_TAIL"]
    assert "SIGNATURES" in tables and len(tables) >= 8
    for table in tables:
        assert not NAMES & set(getattr(_lib, table)), table


def test_the_model_has_the_switch():
    from resdepth_amd import UNet
    assert UNet(n_input_channels=1, start_kernel=16, depth=1).fold_tail_skip is True
