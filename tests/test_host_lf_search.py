"""-av1mi_lf_search in a transcode job: what the session is opened with (host/backend.cpp SessionConfig), the refusal of other values
and the usage text, without a GPU."""
import os

import pytest

from test_host_session_config import BASE, HOST, _config, _expect, _y4m, host      # noqa: F401  (host: the module's fixture)


def test_the_option_reaches_the_session_and_nothing_else_changes(host, tmp_path):
    src = _y4m(tmp_path / "a.y4m", 192, 136, 10)
    code, cfg, target, sw, err = _config(host, src, "-av1mi_lf_search", "1")
    assert code == 0 and err == ""
    _expect(cfg, **dict(BASE, width=192, height=136, lf_search=1))
    code, off, _, _, _ = _config(host, src, "-av1mi_lf_search", "0")
    code2, plain, _, _, _ = _config(host, src)
    assert code == 0 and code2 == 0 and off == plain and plain["lf_search"] == 0


def test_the_option_stands_beside_the_other_searches(host, tmp_path):
    src = _y4m(tmp_path / "a.y4m", 192, 136, 10)
    code, cfg, _, _, err = _config(host, src, "-av1mi_lf_search", "1", "-av1mi_cdef_search", "2", "-av1mi_lr_search", "1")
    assert code == 0 and err == ""
    _expect(cfg, **dict(BASE, width=192, height=136, lf_search=1, cdef_search=2, lr_search=1))


@pytest.mark.parametrize("value", ["2", "-1", "on", "1.0"])
def test_values_other_than_0_and_1_are_refused(host, tmp_path, value):
    src = _y4m(tmp_path / "a.y4m", 64, 48, 4)
    code, _, _, _, err = _config(host, src, "-av1mi_lf_search", value)
    assert code != 0 and "Invalid argument" in err and "-av1mi_lf_search takes 0 or 1" in err


def test_the_usage_text_names_the_option():
    text = open(os.path.join(os.path.dirname(HOST), "main.cpp")).read().split("#include")[0]
    assert "-av1mi_lf_search 0 | 1" in text and " lf:<luma vertical level>/<chroma level>" in text
