"""-av1mi_cdef_search in a transcode job: what the session is opened with (host/backend.cpp SessionConfig), without a GPU."""
import pytest

from test_host_session_config import BASE, _config, _expect, _y4m, host      # noqa: F401  (host: the module's fixture)


@pytest.mark.parametrize("n", [1, 2, 3])
def test_the_option_reaches_the_session_and_nothing_else_changes(host, tmp_path, n):
    src = _y4m(tmp_path / "a.y4m", 192, 136, 10)
    code, cfg, target, sw, err = _config(host, src, "-av1mi_cdef_search", str(n))
    assert code == 0 and err == ""
    _expect(cfg, **dict(BASE, width=192, height=136, cdef_search=n))


def test_zero_is_the_default(host, tmp_path):
    src = _y4m(tmp_path / "a.y4m", 192, 136, 10)
    code, off, _, _, _ = _config(host, src, "-av1mi_cdef_search", "0")
    code2, plain, _, _, _ = _config(host, src)
    assert code == 0 and code2 == 0 and off == plain and plain["cdef_search"] == 0


@pytest.mark.parametrize("value", ["4", "-1", "on", "1.0"])
def test_values_outside_0_to_3_are_refused(host, tmp_path, value):
    src = _y4m(tmp_path / "a.y4m", 64, 48, 4)
    code, _, _, _, err = _config(host, src, "-av1mi_cdef_search", value)
    assert code != 0 and "Invalid argument" in err and "-av1mi_cdef_search takes 0, 1, 2 or 3" in err
