"""The switch table of tests/fused_switches.py against the package: every listed switch exists, ships at the value the
table calls optimised, and the context manager sets and restores all of them."""
import pytest

from fused_switches import SWITCHES, fused_switches, resolved


def test_every_listed_switch_exists_and_ships_optimised():
    table = resolved()
    assert len(table) == len(SWITCHES) == len({(m, n) for m, n, _, _ in SWITCHES})
    for mod, name, shipped, plain in table:
        assert getattr(mod, name) == shipped, (mod.__name__, name, getattr(mod, name))
        assert shipped != plain, (mod.__name__, name)


@pytest.mark.parametrize("on", [True, False])
def test_context_manager_sets_every_switch_and_restores_it(on):
    table = resolved()
    before = [getattr(mod, name) for mod, name, _, _ in table]
    with fused_switches(on):
        for mod, name, shipped, plain in table:
            assert getattr(mod, name) == (shipped if on else plain), (mod.__name__, name)
    assert [getattr(mod, name) for mod, name, _, _ in table] == before
    with pytest.raises(RuntimeError):
        with fused_switches(on):
            raise RuntimeError("restored on the way out as well")
    assert [getattr(mod, name) for mod, name, _, _ in table] == before


def test_a_missing_switch_is_an_error(monkeypatch):
    import fused_switches as FS
    monkeypatch.setattr(FS, "SWITCHES", FS.SWITCHES + (("monosowa_amd.pointwise", "NO_SUCH_SWITCH", True, False),))
    with pytest.raises(AssertionError, match="NO_SUCH_SWITCH"):
        with FS.fused_switches(False):
            pass
