"""The export surface of libpt_amd.so: the unmangled pt_* functions it defines are exactly the functions include/pt_amd.h declares.
Helpers shared between the library's translation units live in C++ namespaces or take C++ linkage, so their names are mangled and
never show up here; a helper that leaks as a plain pt_* symbol, or a declared function that nobody defines, fails this test."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "cosc_4397_pathtracing_raytracing_project_amd", "libpt_amd.so")
HEADER = os.path.join(ROOT, "include", "pt_amd.h")

# defined by the library without a declaration in the header, or the reverse: none
EXCEPTIONS: set = set()


def declared() -> set:
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    # a declaration: a return type at the start of a line, the name, an opening parenthesis
    return set(re.findall(r"^[A-Za-z_][\w \t\*]*?\b(pt_\w+)\s*\(", text, flags=re.M))


def defined() -> set:
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB], text=True)
    names = set()
    for line in out.splitlines():
        parts = line.split()
        if len(parts) == 3 and parts[1] in "TtWw" and parts[2].startswith("pt_"):
            names.add(parts[2].split("@")[0])
    return names


def test_exports_equal_header():
    if not os.path.exists(LIB):
        pytest.skip("libpt_amd.so has not been built")
    if not shutil.which("nm"):
        pytest.skip("no nm on this machine")
    want, got = declared(), defined()
    assert len(want) > 100, sorted(want)  # the parser found the header's declarations
    assert got - want - EXCEPTIONS == set(), "defined but not declared in pt_amd.h"
    assert want - got - EXCEPTIONS == set(), "declared in pt_amd.h but not defined"
