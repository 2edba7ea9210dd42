"""The C-ABI library loads and exports every symbol include/tempest_hip.h declares (no GPU needed)."""


def declared_symbols():
    from tempest_amd import _lib
    from tempest_amd._cdecl import prototypes
    with open(_lib.HEADER_PATH) as f:
        return sorted(prototypes(f.read(), "tph_"))


def test_library_exports_header():
    from tempest_amd import _lib
    lib = _lib.load()
    names = declared_symbols()
    assert len(names) >= 30
    for n in names:
        assert hasattr(lib, n), n
    assert set(names) == set(_lib.SIGNATURES), set(names) ^ set(_lib.SIGNATURES)
    assert lib.tph_version() == 100
    assert lib.tph_version() == _lib.CONSTANTS["TPH_VERSION"]


def test_missing_library_fails_loudly(tmp_path):
    import pytest
    from tempest_amd import _lib
    with pytest.raises(_lib.TempestHipError):
        _lib.load(str(tmp_path / "nope.so"))
