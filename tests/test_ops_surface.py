"""idgrec_amd.ops is a package of one module per kernel family: every attribute of it that the tree writes must resolve, module
state must be one object however it is reached, and no module of the package may import the package."""
import glob
import importlib
import os
import re
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "id-grec_amd", "ops")
# the private names the engines, the models, bench.py and the tests reach through the package
PRIVATE = ("_stream", "_next_noise_stream", "_check_groups", "_require_device", "_tnce_ws_cache", "_kmeans_ws_cache",
           "_compose_views", "_noise_stream", "_ssl_ws")
IMPORTS_OPS = re.compile(r"^\s*(import idgrec_amd\.ops\b|from idgrec_amd import [^\n]*\bops\b|from \.+ import [^\n]*\bops\b)", re.M)
USES = re.compile(r"\bops\.([A-Za-z_]\w*)")


@pytest.fixture(scope="module")
def ops():
    import idgrec_amd.ops as ops_  # (no device needed: the package only loads the library)

    return ops_


def _sources():
    files = [os.path.join(ROOT, f) for f in ("bench.py", "__graft_entry__.py", "main.py")]
    for d in ("id-grec_amd", "models", "utility", "tests", "scripts"):
        files += glob.glob(os.path.join(ROOT, d, "**", "*.py"), recursive=True)
    return sorted(f for f in files if os.path.isfile(f) and not f.startswith(PKG + os.sep))


def test_every_ops_name_written_in_the_tree_resolves(ops):
    seen, missing = 0, []
    for path in _sources():
        text = open(path, encoding="utf-8").read()
        if not IMPORTS_OPS.search(text):  # `ops` is a fixture argument or a local there, not necessarily this package
            continue
        for name in sorted(set(USES.findall(text))):
            seen += 1
            if not hasattr(ops, name):
                missing.append("%s: ops.%s" % (os.path.relpath(path, ROOT), name))
    assert seen > 100 and not missing, missing


def test_names_are_the_defining_module_s_objects(ops):
    """A state list or cache that was copied into the package instead of re-exported would pass every other test."""
    subs = {n: importlib.import_module("idgrec_amd.ops." + n)
            for n in (os.path.basename(f)[:-3] for f in glob.glob(os.path.join(PKG, "*.py"))) if n != "__init__"}
    assert sorted(set(ops.__all__)) == sorted(ops.__all__)
    for name in tuple(ops.__all__) + PRIVATE:
        obj = getattr(ops, name)
        if isinstance(obj, (types.FunctionType, type)):
            homes = [m for m in subs.values() if m.__name__ == obj.__module__]
        else:  # constants and state: the one submodule that assigns the name at its top level
            homes = [m for n, m in subs.items()
                     if re.search(r"^(?:[A-Za-z_][\w, ]*, )?%s(?:, [\w, ]*)? = " % re.escape(name), open(m.__file__).read(), re.M)]
        assert len(homes) == 1, (name, [m.__name__ for m in homes])
        assert getattr(homes[0], name) is obj, name
    assert ops._compose_views == [False] and isinstance(ops._noise_stream, list)


def test_no_module_of_the_package_imports_the_package():
    for path in glob.glob(os.path.join(PKG, "*.py")):
        text = open(path, encoding="utf-8").read()
        assert not re.search(r"import idgrec_amd\.ops|from \.\. import [^\n]*\bops\b|from idgrec_amd import [^\n]*\bops\b", text), path
