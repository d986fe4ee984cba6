"""csrc/launchers.h is the single declaration of the kernels' C ABI (text-only checks, no build).

Every pdt_* launcher a .hip file defines is declared in the header, every declaration there has
exactly one definition, and binding.cpp carries no prototype of its own: the header, included by both
sides, is what turns a changed parameter list into a compile error instead of a bad call.
"""
import glob
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "pytorch_distributed_training_example_amd", "csrc")

# a definition or declaration at the start of a line; `static` helpers do not match. conv_stem.hip marks
# each launcher `extern "C"` on its own line instead of wrapping them in a block.
_FUNC = re.compile(r'^[ \t]*(?:extern "C"[ \t]+)?(int|int64_t|void)\s+(pdt_\w+)\(', re.M)


def _read(*parts):
    with open(os.path.join(CSRC, *parts)) as f:
        return f.read()


def _defined():
    """name -> [the .hip files that define it]"""
    out = {}
    for path in sorted(glob.glob(os.path.join(CSRC, "kernels", "*.hip"))):
        for _, name in _FUNC.findall(_read(path)):
            out.setdefault(name, []).append(os.path.basename(path))
    return out


def _declared():
    return [name for _, name in _FUNC.findall(_read("launchers.h"))]


def test_every_launcher_is_declared_in_the_header():
    defined, declared = _defined(), set(_declared())
    assert len(defined) > 100  # the scan sees the kernels
    missing = sorted(set(defined) - declared)
    assert not missing, f"defined in a .hip but not declared in launchers.h: {missing}"


def test_every_declaration_has_exactly_one_definition():
    defined, declared = _defined(), _declared()
    assert len(declared) == len(set(declared)), "a launcher is declared twice in launchers.h"
    bad = {n: defined.get(n, []) for n in declared if len(defined.get(n, [])) != 1}
    assert not bad, f"declared in launchers.h but not defined in exactly one .hip: {bad}"


def test_every_kernel_file_includes_the_header():
    for path in sorted(glob.glob(os.path.join(CSRC, "kernels", "*.hip"))):
        assert '#include "../launchers.h"' in _read(path), os.path.basename(path)


def test_header_is_torch_free():
    includes = re.findall(r"^#include\s+(\S+)", _read("launchers.h"), re.M)
    assert includes == ["<hip/hip_runtime.h>", "<stdint.h>"]
    assert "#pragma once" in _read("launchers.h")


def test_binding_has_no_prototypes_of_its_own():
    src = _read("binding.cpp")
    assert '#include "launchers.h"' in src
    assert 'extern "C"' not in src
    assert not re.search(r"\b(int|int64_t|void)\s+pdt_\w+\s*\(", src)
