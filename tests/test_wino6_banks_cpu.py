"""CPU: the exchange buffer of the F(6x6) output stage (csrc/b2f_wino6.hip) lane by lane -- tools/wino6_banks.py enumerates the LDS bank of
every lane of every write of the dump and every read of the rounds.  Pure arithmetic: the shipped form ("rows") has no bank conflict in
either direction, its reads find every half where the dump put it, and the items of a parity cover the 48 x 12 pixels x 32 outputs once."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("wino6_banks", os.path.join(ROOT, "tools", "wino6_banks.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_shipped_exchange_layout_is_conflict_free_and_consistent():
    t = _tool()
    assert t.worst_degrees("rows") == (1, 1)
    assert t.roundtrip_ok("rows")


def test_first_layout_had_two_way_conflicts():
    """the form the kernel started with, kept in the tool as the comparison: 2-way on reads and writes (what the SQ counters showed)"""
    t = _tool()
    assert t.worst_degrees("plain") == (2, 2)
    assert t.roundtrip_ok("plain")


def test_tool_constants_match_the_kernel():
    src = open(os.path.join(ROOT, "back2future_amd", "csrc", "b2f_wino6.hip")).read()
    assert "constexpr int XPS = %d;" % _tool().XPS in src
