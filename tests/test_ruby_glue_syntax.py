"""The Ruby-side glue has never met a Ruby toolchain (the image has none): at least the C compiler's FRONT END
sees it.  `gcc -fsyntax-only -std=c99 -Wall -Wextra -Werror` over

  * ruby/ext/blurrily/map_ext_reference.c -- the gem's OWN glue (ext/blurrily/map_ext.c:1-230), #included where
    it lies in the reference tree with its initialiser renamed, and
  * ruby/ext/blurrily/map_ext_batch.c -- the batched methods, against the gem's storage.h AND
    include/blurrily_storage.h in one translation unit,

with the declarations-only headers of tests/c/mock_ruby/ in place of ruby.h.  No object code is produced and
nothing is linked or run.  A second check holds the two translation units to ONE definition of Init_map_ext
(what the rename is for): the preprocessed gem glue must define Init_map_ext_reference and not Init_map_ext.

The gem's storage.h is the stand-in helpers.write_recorded_storage_h makes from tests/golden/ref_abi.json, and
where the gem's map_ext.c is needed as a whole a stand-in holds what ref_abi.json recorded of it (its initialiser,
the methods it defines).  Only the front-end pass over the gem's own glue needs the gem's sources themselves: it
runs where $BLURRILY_GEM_EXT (as in extconf.rb) or the reference tree holds them."""
import os
import re
import subprocess

import pytest

import helpers
from helpers import load_golden, write_recorded_storage_h

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEM_EXT = os.environ.get("BLURRILY_GEM_EXT", "/root/reference/ext/blurrily")
MOCK = os.path.join(ROOT, "tests", "c", "mock_ruby")
GLUE = os.path.join(ROOT, "ruby", "ext", "blurrily")
# the gem's own flags (ext/blurrily/extconf.rb:4-16), -Werror kept: the glue must be warning-free
FLAGS = [*helpers.FLAGS, "-I", MOCK]
INCLUDE = ["-I", os.path.join(ROOT, "include")]
ABI = load_golden("ref_abi.json")


def _gcc(*args):
    return subprocess.run(["gcc", *args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def _recorded_gem(directory):
    """-I flags of a directory standing in for the gem's ext/blurrily: the recorded storage.h, and a map_ext.c that
    defines the gem's recorded initialiser and nothing else"""
    write_recorded_storage_h(directory)
    with open(os.path.join(str(directory), "map_ext.c"), "w") as f:
        f.write('#include "storage.h"\n%s;\n%s { }\n' % (ABI["gem_initialiser"], ABI["gem_initialiser"]))
    return ["-I", str(directory)] + INCLUDE


@pytest.mark.parametrize("src", ["map_ext_reference.c", "map_ext_batch.c"])
def test_glue_passes_the_front_end(src, tmp_path):
    if src == "map_ext_reference.c":
        # the gem's own glue, #included where it lies: nothing but the gem's sources can stand in for it
        if not os.path.exists(os.path.join(GEM_EXT, "map_ext.c")):
            pytest.skip("the gem's map_ext.c is not here (set BLURRILY_GEM_EXT to the gem's ext/blurrily)")
        inc = ["-I", GEM_EXT] + INCLUDE
    else:
        inc = _recorded_gem(tmp_path)
    res = _gcc("-fsyntax-only", *FLAGS, *inc, os.path.join(GLUE, src))
    assert res.returncode == 0, res.stdout


def test_one_definition_of_the_initialiser(tmp_path):
    inc = _recorded_gem(tmp_path)
    ref = _gcc("-E", "-P", *FLAGS, *inc, os.path.join(GLUE, "map_ext_reference.c"))
    bat = _gcc("-E", "-P", *FLAGS, *inc, os.path.join(GLUE, "map_ext_batch.c"))
    assert ref.returncode == 0 and bat.returncode == 0, ref.stdout + bat.stdout
    defines = lambda text, name: re.search(r"\bvoid\s+%s\s*\(\s*void\s*\)\s*\{" % name, text) is not None
    assert defines(ref.stdout, "Init_map_ext_reference") and not defines(ref.stdout, "Init_map_ext")
    assert defines(bat.stdout, "Init_map_ext") and not defines(bat.stdout, "Init_map_ext_reference")
    # ... and the batch glue calls the gem's initialiser first
    assert re.search(r"Init_map_ext_reference\s*\(\s*\)\s*;", bat.stdout)


def test_the_mock_headers_define_nothing():
    """declarations only: no function body, no object definition (a stand-in Ruby would be something else)"""
    for rel in ("ruby.h", os.path.join("ruby", "thread.h")):
        text = open(os.path.join(MOCK, rel)).read()
        text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
        body = re.sub(r"struct\s+\w+\s*\{[^}]*\}\s*;", "", text)          # a struct's fields are not a body
        body = re.sub(r"enum\s+\w+\s*\{[^}]*\}\s*;", "", body)
        assert "{" not in body, rel


def test_every_guarded_method_exists_in_the_gem():
    """the wrappers re-define exactly methods the gem's Init_map_ext defines (map_ext.c:219-228, as recorded in
    tests/golden/ref_abi.json)"""
    batch = open(os.path.join(GLUE, "map_ext_batch.c")).read()
    guarded = re.findall(r'guard_method\("(\w+)"', batch)
    assert sorted(guarded) == ["close", "delete", "find", "put", "save", "stats"]
    for name in guarded:
        assert name in ABI["gem_methods"], name
