"""Builds and loads the C checkers under tests/ -- TEST INFRASTRUCTURE ONLY.

Every checker is one C source built with oracle/Makefile's CC and CFLAGS into tests/_build/ on first use, or when its
source, one of the sources it includes, or any of the oracle's is newer than the library.
"""
from __future__ import annotations

import ctypes as ct
import os
import re
import shlex
import subprocess

import oracle_ref as orc

HERE = os.path.dirname(os.path.abspath(__file__))
BUILD_DIR = os.path.join(HERE, "_build")


def _make_vars():
    """CC and CFLAGS as oracle/Makefile sets them (CC ?= ..., so the environment's CC wins)"""
    text = open(os.path.join(orc.ORACLE_DIR, "Makefile")).read()
    cc = re.search(r"^CC\s*\?=\s*(.+)$", text, re.M).group(1).strip()
    cflags = re.search(r"^CFLAGS\s*:=\s*(.+)$", text, re.M).group(1).strip()
    return os.environ.get("CC", cc), shlex.split(cflags)


def load(src, lib_name, extra_deps=()):
    """the CDLL of tests/<src>, rebuilt first (into a temporary name, then renamed) when stale; extra_deps: the files
    under tests/ that src includes"""
    path = os.path.join(BUILD_DIR, lib_name)
    deps = [os.path.join(HERE, f) for f in (src, *extra_deps)]
    deps += [os.path.join(orc.ORACLE_DIR, f) for f in os.listdir(orc.ORACLE_DIR) if f.endswith((".c", ".h", ".inc"))]
    if not os.path.exists(path) or any(os.path.getmtime(p) > os.path.getmtime(path) for p in deps):
        cc, cflags = _make_vars()
        os.makedirs(BUILD_DIR, exist_ok=True)
        tmp = path + f".{os.getpid()}.tmp"
        subprocess.run([cc, *cflags, "-shared", "-o", tmp, src, "-lm"], check=True, cwd=HERE)
        os.replace(tmp, path)
    return ct.CDLL(path)
