"""The contract of the C ABI, stated once for every public header (`_lib.TABLES`): a header's declarations, its ctypes table,
what `load()` bound and what libmdno.so exports agree; no name stands in two tables; the library exports nothing that starts
with mdno beyond the tables; include/ holds the registry's headers and no other; and the build id covers every one of them.
No GPU needed, no compute calls.

The per-prefix statements the tests of the single headers used to make follow from three things checked here and one pinned
there: with `set(table) == NAMES` in a header's own test file, global export equality gives
`{n in exported : n.startswith(prefix)} == set(decls)` for that header's prefix, and disjointness from every other table
together with the other files' NAMES gives `not any(n.startswith(prefix) for n in others)`."""
import hashlib
import re
import shutil

import pytest

from cabi import CSRC, INCLUDE, declared_functions, exported_symbols, lib  # noqa: F401  (lib: the fixture)
from molecular_dynamics_neural_operator_amd import _lib

HEADERS = [h for h, _ in _lib.TABLES]


@pytest.mark.parametrize("header,table", _lib.TABLES, ids=HEADERS)
def test_header_table_bindings_and_exports_agree(lib, header, table):
    decls = declared_functions(INCLUDE / header)
    assert decls, f"{header} declares nothing the parser sees"
    undeclared, untabled = sorted(set(table) - set(decls)), sorted(set(decls) - set(table))
    assert not undeclared and not untabled, f"{header}: in the table but not declared {undeclared}; declared without a table entry {untabled}"
    exported = exported_symbols()
    for name, (res, args) in table.items():
        assert len(args) == decls[name], f"{name}: the table has {len(args)} argtypes, {header} declares {decls[name]} parameters"
        fn = getattr(lib, name)
        assert fn.argtypes == args and fn.restype == res, f"{name}: load() did not bind the signature of {header}'s table"
        assert name in exported, f"{name} is declared in {header} but libmdno.so does not export it"
    for other, other_table in _lib.TABLES:
        shared = sorted(set(table) & set(other_table)) if other != header else []
        assert not shared, f"{shared} stand in the tables of {header} and of {other}"


def test_the_merged_mapping_is_the_union_and_refuses_a_name_in_two_tables():
    assert set(_lib.BINDINGS) == set().union(*(t for _, t in _lib.TABLES))
    assert len(_lib.BINDINGS) == sum(len(t) for _, t in _lib.TABLES)
    assert len(set(HEADERS)) == len(HEADERS)
    twice = _lib.TABLES + (("mdno_again.h", {"mdno_noise_fill": _lib.NOISE_SIGNATURES["mdno_noise_fill"]}),)
    with pytest.raises(_lib.MdnoError, match="mdno_noise_fill stands in the tables of mdno_noise.h and of mdno_again.h"):
        _lib.merge_tables(twice)


def test_the_library_exports_the_tables_and_nothing_else(lib):
    """For every prefix at once: nothing exported undeclared, nothing declared unexported."""
    exported = {n for n in exported_symbols() if n.startswith("mdno")}
    extra, missing = sorted(exported - set(_lib.BINDINGS)), sorted(set(_lib.BINDINGS) - exported)
    assert not extra and not missing, f"exported without a table entry {extra}; in a table but not exported {missing}"


def test_include_holds_the_registrys_headers_and_no_other():
    present = {f.name for f in INCLUDE.iterdir() if f.suffix == ".h"}
    extra, missing = sorted(present - set(HEADERS)), sorted(set(HEADERS) - present)
    assert not extra and not missing, f"in include/ without a line in _lib.TABLES {extra}; in _lib.TABLES but not in include/ {missing}"


def recomputed_id():
    files = sorted([f for f in CSRC.iterdir() if f.suffix in (".hip", ".h", ".sh")], key=lambda f: str(f).encode())
    files += [INCLUDE / name for name in sorted(HEADERS, key=str.encode)]
    return hashlib.sha256(b"".join(f.read_bytes() for f in files)).hexdigest()[:16]


def test_the_build_id_is_the_hash_of_csrc_and_every_header(lib):
    want = _lib.source_build_id()
    assert want is not None and len(want) == 16
    assert want == recomputed_id(), "source_build_id() is not sha256 over csrc/*.{hip,h,sh} + the registry's headers"
    assert lib.mdno_build_id().decode() == want, "the library was built from other sources"
    assert (CSRC / "build" / "BUILD_ID").read_text().split()[0] == want, "build.sh and source_build_id() form different ids"
    named = re.findall(r"mdno\w*\.h", (CSRC / "build.sh").read_text())
    assert not named, f"build.sh names single headers {named}: it takes include/*.h"


def test_a_byte_in_any_header_moves_the_build_id(tmp_path):
    shutil.copytree(INCLUDE, tmp_path / "include")
    shutil.copytree(CSRC, tmp_path / CSRC.parent.name / "csrc", ignore=shutil.ignore_patterns("build"))
    before = _lib.source_build_id(tmp_path)
    assert before == _lib.source_build_id()
    for header in HEADERS:          # (mdno_markov.h among them)
        path = tmp_path / "include" / header
        kept = path.read_bytes()
        path.write_bytes(kept + b"/**/")
        assert _lib.source_build_id(tmp_path) != before, f"a comment appended to {header} leaves the build id as it was"
        path.write_bytes(kept)
        assert _lib.source_build_id(tmp_path) == before
    (tmp_path / "include" / "mdno_markov.h").unlink()
    assert _lib.source_build_id(tmp_path) is None
