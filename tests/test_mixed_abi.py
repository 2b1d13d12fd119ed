"""CPU tests of the mixed-robot tick's C boundary (include/osc_mixed.h): the header's declarations
are the symbols _lib.MIXED_SYMBOLS lists and the library exports, the ABI version is unchanged,
argument errors are reported without a device, and the ctypes structures have the layout the C
compiler gives the header's."""
import ctypes
import gc
import os
import re
import shutil
import subprocess
import weakref

import numpy as np
import pytest

from osc_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "osc_mixed.h")


def test_header_declarations_are_the_exported_symbols():
    L = _lib.lib()
    declared = set(re.findall(r"^\s*(?:int|void|const char\*)\s+(osc_\w+)\s*\(", open(HEADER).read(),
                              re.M))
    assert declared == set(_lib.MIXED_SYMBOLS)
    for name in declared:
        assert hasattr(L, name), name
    assert not declared & set(_lib.EXPORTED_SYMBOLS) and not declared & set(_lib.ROLLOUT_SYMBOLS)
    assert L.osc_abi_version() == 4          # additive: ABI 4 callers are untouched


def test_bad_arguments_without_a_device():
    L = _lib.lib()
    vp = ctypes.c_void_p
    assert L.osc_batch_tick_multi(None, 1, None) == 1
    assert L.osc_batch_tick_multi(None, -1, None) == 1
    assert L.osc_batch_tick_multi(None, 0, None) == 0          # nothing to do
    jobs = (_lib.OscTickJob * 2)()                             # NULL models
    assert L.osc_batch_tick_multi(jobs, 2, None) == 1
    assert L.osc_batch_kinematics_pair(*([None, 1] + [None] * 6) * 2, None) == 1
    h = vp()
    parts = (_lib.OscFeedPart * 3)()
    for n in (0, 1, 2, 3):                                     # no parts / NULL models / three parts
        assert L.osc_host_feed_create_multi(parts, n, 0, 0, 2, ctypes.byref(h)) == 1
    assert L.osc_host_feed_create_multi(None, 1, 0, 0, 2, ctypes.byref(h)) == 1
    assert L.osc_host_feed_create_multi(parts, 1, 0, 0, 2, None) == 1
    i, o = _lib.OscFeedInputs(), _lib.OscFeedOutputs()
    assert L.osc_host_feed_inputs_part(None, 0, 0, ctypes.byref(i)) == 1
    assert L.osc_host_feed_wait_part(None, 0, 0, ctypes.byref(o)) == 1


C_PROGRAM = r"""
#include <stddef.h>
#include <stdio.h>
#include "osc_mixed.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(osc_tick_job), offsetof(osc_tick_job, nenv),
         offsetof(osc_tick_job, M), offsetof(osc_tick_job, qpos), offsetof(osc_tick_job, tau),
         offsetof(osc_tick_job, warm_state_bytes), offsetof(osc_tick_job, workspace_bytes),
         sizeof(osc_feed_part));
  return 0;
}
"""


def test_structures_match_the_c_layout(tmp_path):
    """sizeof / offsetof as a C compiler sees include/osc_mixed.h (a C header: compiled as C)."""
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc is not None, "no C compiler"
    src = tmp_path / "layout.c"
    src.write_text(C_PROGRAM)
    exe = tmp_path / "layout"
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"),
                    str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True,
                                          text=True).stdout.split()]
    J = _lib.OscTickJob
    assert got == [ctypes.sizeof(J), J.nenv.offset, J.M.offset, J.qpos.offset, J.tau.offset,
                   J.warm_state_bytes.offset, J.workspace_bytes.offset,
                   ctypes.sizeof(_lib.OscFeedPart)]


def test_feed_views_keep_their_owner_alive():
    """MixedHostFeed's views refer to the object that owns the native feed (no use-after-free when
    the feed object goes first): the view helper's base chain holds the owner."""
    from osc_amd.host_feed import _owned_view

    class Owner:
        pass

    owner = Owner()
    alive = weakref.ref(owner)
    buf = (ctypes.c_double * 6)(*range(6))
    view = _owned_view(owner, ctypes.addressof(buf), (2, 3))[1]     # a view of the view
    del owner
    gc.collect()
    assert alive() is not None
    assert np.array_equal(view, [3.0, 4.0, 5.0])
    del view
    gc.collect()
    assert alive() is None
