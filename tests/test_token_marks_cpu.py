"""CPU: token timing marks (include/kokorox_hip.h, "token marks") -- the numpy mirror of kokorox_amd/voices.py against known
answers written out by hand, the host layout of the marks block (kokorox_amd/csrc/host_request.cpp: build_output_plan,
output_bounds, check_marks_call) through tests/cpp/marks_plan_check.cpp, built with g++ -fsanitize=address,undefined and run
as a child process (nothing is loaded into python), and the names of the new entries in the bindings.
"""
import os
import re
import subprocess

import numpy as np
import pytest

from kokorox_amd import voices as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATES = {0x000: 600, 0x100: 200, 0x200: 400, 0x300: 1200}  # the rate of a format word -> K = 600 L / M
NULL_MARKS = "infer: null marks argument"


# ---- the numpy mirror ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", sorted(RATES))
def test_known_answers_of_a_two_chunk_request(rate):
    """durations [2, 1] and [1, 3, 1]: frames before each token 0 2 | 3 and 3 4 7 | 8; by hand at every rate."""
    by_hand = {
        0x000: [0, 1200, 1800, 1800, 2400, 4200, 4800],
        0x100: [0, 400, 600, 600, 800, 1400, 1600],
        0x200: [0, 800, 1200, 1200, 1600, 2800, 3200],
        0x300: [0, 2400, 3600, 3600, 4800, 8400, 9600],
    }[rate]
    for form in (0, 1, 2, 3, 4, 8, 9):  # samples, not bytes: the form does not matter
        m = V.token_marks([[2, 1], [1, 3, 1]], form | rate)
        assert m.dtype == np.int64
        assert m.tolist() == by_hand
    assert by_hand[-1] == RATES[rate] * 8 and by_hand[2] == by_hand[3]  # the request's samples; the boundary, stored twice
    spans = V.token_spans(by_hand, [2, 3])
    assert [s.tolist() for s in spans[0]] == [by_hand[0:2], by_hand[1:3]]
    assert [s.tolist() for s in spans[1]] == [by_hand[3:6], by_hand[4:7]]
    # words as token ranges: the first chunk as one word, the middle token of the second, its last two
    assert V.word_spans(spans[0], [(0, 1)]) == [(0, by_hand[2])]
    assert V.word_spans(spans[1], [(1, 1), (1, 2)]) == [(by_hand[4], by_hand[5]), (by_hand[4], by_hand[6])]


@pytest.mark.parametrize("rate", sorted(RATES))
def test_known_answer_of_a_single_token_chunk(rate):
    assert V.token_marks([[7]], rate).tolist() == [0, 7 * RATES[rate]]
    assert V.token_marks([[1]], 8 | rate).tolist() == [0, RATES[rate]]
    (start, end), = V.token_spans(V.token_marks([[7]], rate), [1])
    assert start.tolist() == [0] and end.tolist() == [7 * RATES[rate]]


def test_mirror_is_64_bit_and_refuses_what_has_no_marks():
    m = V.token_marks([[4096] * 512, [4096] * 512], 0x300)
    assert int(m[-1]) == 2 * 512 * 4096 * 1200 == 5033164800 and m.shape == (1026,)
    assert (np.diff(m[:513]) == 4096 * 1200).all() and m[512] == m[513]
    for bad in (lambda: V.token_marks([], 0), lambda: V.token_marks([[1], []], 0), lambda: V.token_marks([[1]], 0x400),
                lambda: V.token_spans([0, 1, 2], [3]), lambda: V.word_spans(([0, 1], [1, 2]), [(1, 2)]),
                lambda: V.word_spans(([0, 1], [1, 2]), [(1, 0)])):
        with pytest.raises(ValueError):
            bad()


# ---- the host layout (HIP-free, under the sanitizers) ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("marks_plan") / "marks_plan_check")
    csrc = os.path.join(ROOT, "kokorox_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc,
                    os.path.join(ROOT, "tests", "cpp", "marks_plan_check.cpp"), os.path.join(csrc, "host_request.cpp"),
                    "-o", exe], check=True)

    def run(mode):
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
        r = subprocess.run([exe, mode], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]  # (a sanitizer report aborts the driver)
        return r.stdout
    return run


def test_mark_plans_and_the_packed_bound(driver):
    """Counts, the block's offset (8-aligned, at or after the bodies) and every row's base for the groupings [1]*6, [2,1,3], [6]
    in every form and rate, with all / none / some / null want flags (rows that are not wanted get -1); the packed bound (output_bounds)
    unchanged without marks and large enough with them at one frame per token.  The driver compares with sums of its own."""
    out = driver("plans")
    print(out)
    assert "mark plans: 339 (grouping, words, want) cases over 6 rows" in out
    assert "bounds: 168 batches of one frame per token" in out


def test_refusals_of_the_marks_arguments(driver):
    got = dict(line.split("\t", 1) for line in driver("refusals").splitlines())
    assert got == {
        "null_out_marks": "1\t" + NULL_MARKS,
        "null_out_n_marks": "1\t" + NULL_MARKS,
        "marks_without_requests": "1\tinfer: marks are for requests (chunks_per_request)",
        "ok": "accepted",
    }


# ---- the ABI ----------------------------------------------------------------------------------------------------------
def test_the_new_entries_are_part_of_the_abi():
    from kokorox_amd import hip_koko as hk
    assert "kx_infer_requests_marks" in hk.ABI_SYMBOLS
    assert "kx_dispatcher_submit_request_marks" in hk.ABI_SYMBOLS
    assert "kx_test_output_plan" in hk.TEST_ABI_SYMBOLS
    assert "kx_test_output_plan" not in hk.ABI_SYMBOLS  # (the hook lives in the test library only)
    header = open(os.path.join(ROOT, "include", "kokorox_hip.h"), encoding="utf-8").read()
    test_header = open(os.path.join(ROOT, "include", "kokorox_hip_test.h"), encoding="utf-8").read()
    for name in ("kx_infer_requests_marks", "kx_dispatcher_submit_request_marks"):
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name not in test_header
    assert re.search(r"^int kx_test_output_plan\(", test_header, re.M) and "kx_test_output_plan" not in header
    # the refusal texts the GPU suite matches are the ones the header promises
    assert '"%s"' % NULL_MARKS in header and '"dispatcher_submit_request: null marks argument"' in header


def test_header_restates_the_definition():
    header = open(os.path.join(ROOT, "include", "kokorox_hip.h"), encoding="utf-8").read()
    for phrase in ("m_c[t] = K * (", "K = 600 L / M", "[m_c[t], m_c[t+1])", "m_c[T_c] = m_{c+1}[0]", "out_samples[r]",
                   "symmetric about its tap C", "SAMPLES of the stream, not bytes"):
        assert phrase in header, phrase
