"""-av1mi_lr_search in a transcode job: what the session is opened with (host/backend.cpp SessionConfig), without a GPU."""
import pytest

from test_host_session_config import BASE, _config, _expect, _y4m, host      # noqa: F401  (host: the module's fixture)


def test_the_option_reaches_the_session_and_nothing_else_changes(host, tmp_path):
    src = _y4m(tmp_path / "a.y4m", 192, 136, 10)
    code, cfg, target, sw, err = _config(host, src, "-av1mi_lr_search", "1")
    assert code == 0 and err == ""
    _expect(cfg, **dict(BASE, width=192, height=136, lr_search=1))
    code, off, _, _, _ = _config(host, src, "-av1mi_lr_search", "0")
    code2, plain, _, _, _ = _config(host, src)
    assert code == 0 and code2 == 0 and off == plain and plain["lr_search"] == 0


@pytest.mark.parametrize("value", ["2", "-1", "on", "1.0"])
def test_values_other_than_0_and_1_are_refused(host, tmp_path, value):
    src = _y4m(tmp_path / "a.y4m", 64, 48, 4)
    code, _, _, _, err = _config(host, src, "-av1mi_lr_search", value)
    assert code != 0 and "-av1mi_lr_search takes 0 or 1" in err
