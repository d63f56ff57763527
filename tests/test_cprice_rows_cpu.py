"""CPU: the tier rule of compact pricing's row form (csrc/spx_cprows.h, shared
by k_price and cprice_setup): the chunks and the columns in flight for a list
length, the SPX_CPRICE_ROWS limit clamped to the rows of AS, the LDS of the
slots; and the header constants the additive interface leaves alone."""
import json
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("cprows") / "cprows_check")
    subprocess.run(["g++", "-std=c++17", "-O1", os.path.join(ROOT, "tools", "cprows_check.cpp"), "-o", exe],
                   check=True, timeout=120)

    def run(*args):
        r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=60, check=True)
        return json.loads(r.stdout)

    return run


# S -> (chunks of 64 entries, columns in flight) under the default limit;
# 0 chunks: the gather form, which keeps its two columns
TIERS = {0: (0, 2), 1: (2, 4), 64: (2, 4), 65: (2, 4), 128: (2, 4), 129: (4, 4), 256: (4, 4), 257: (8, 2),
         512: (8, 2), 513: (0, 2)}


@pytest.mark.parametrize("S", sorted(TIERS))
def test_tier_of_list_length(check, S):
    nc, depth = TIERS[S]
    assert check("tier", S, 512) == {"nc": nc, "depth": depth}


def test_tier_under_a_lower_limit(check):
    # the limit is the longest list served: past it the gather form, at any tier
    for limit, S, nc in ((0, 1, 0), (1, 1, 2), (1, 2, 0), (64, 64, 2), (64, 65, 0), (129, 129, 4), (129, 130, 0),
                         (300, 300, 8), (300, 301, 0)):
        assert check("tier", S, limit)["nc"] == nc, (limit, S)
    # a row is never read in more chunks than the slot of its limit holds
    for limit in (1, 63, 64, 65, 128, 129, 256, 257, 512):
        slot = check("lds", 4, limit)["slot_doubles"]
        for S in range(1, limit + 1, 7):
            assert 64 * check("tier", S, limit)["nc"] + 2 <= slot


def test_limit_from_environment(check):
    assert check("limit", "unset", 1024) == {"limit": 512}  # the default
    assert check("limit", "unset", 40) == {"limit": 40}  # clamped to the rows of AS
    assert check("limit", "0", 1024) == {"limit": 0}
    assert check("limit", "65", 1024) == {"limit": 65}
    assert check("limit", "65", 33) == {"limit": 33}
    assert check("limit", "4096", 4096) == {"limit": 512}  # no tier past 8 chunks
    assert check("limit", "x", 1024) == {"limit": 512}  # unparsable: the default
    assert check("limit", "-3", 1024) == {"limit": 512}


def test_limit_steps_down_by_tier(check):
    # cprice_setup lowers the limit to the next smaller slot while the slots
    # would take a workgroup off a CU
    assert [check("below", x, 0)["limit"] for x in (512, 300, 257, 256, 200, 129, 128, 33, 1, 0)] == \
        [256, 256, 256, 128, 128, 128, 0, 0, 0, 0]
    for x in (512, 300, 256, 129):
        assert check("lds", 4, check("below", x, 0)["limit"])["lds_bytes"] < check("lds", 4, x)["lds_bytes"]


def test_lds_bytes(check):
    # a slot: the widest row of the limit and the unit entry's pair
    assert check("lds", 4, 512) == {"slot_doubles": 514, "lds_bytes": 4 * 514 * 8}
    assert check("lds", 8, 512)["lds_bytes"] == 8 * 514 * 8
    assert check("lds", 4, 256) == {"slot_doubles": 258, "lds_bytes": 4 * 258 * 8}
    assert check("lds", 4, 128)["slot_doubles"] == 130
    assert check("lds", 4, 33)["slot_doubles"] == 130
    assert check("lds", 4, 0) == {"slot_doubles": 0, "lds_bytes": 0}
    # three 256-thread workgroups of the default geometry fit a CU's 160 KiB
    # beside cf / cpos / crow at 1,024 stored rows and the partials
    assert 3 * (4 * 514 * 8 + 1024 * 16 + 4 * 32 + 16 + 1024) <= 160 * 1024


def test_header_constants_and_entry_point():
    h = open(os.path.join(ROOT, "include", "simplex.h")).read()
    assert re.search(r"#define\s+SPX_CONFIG_FIELDS\s+17\b", h)
    assert re.search(r"#define\s+SPX_DISPATCH_FIELDS\s+12\b", h)
    assert re.search(r"#define\s+SPX_ABI_VERSION\s+8\b", h)  # additive: the version stays
    assert re.search(r"int\s+spx_cprice_rows\(spx_ctx\*\s*ctx,\s*int32_t\s+out\[2\]\);", h)
    from simplex_method_gpu_amd import _lib

    assert "spx_cprice_rows" in _lib.SIGNATURES
