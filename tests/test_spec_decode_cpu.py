"""Greedy speculative decoding, the parts that need no GPU: the host reference of the draft stage (`host.prompt_lookup_draft`, HF
PromptLookupCandidateGenerator semantics), the accept rule as the header states it, the new C ABI (prototypes on both sides, the layout of
VilaDecodeVerify) and what `generate` refuses before it touches a device."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from vila_amd import _lib, configs
from vila_amd.host import prompt_lookup_draft

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (ids, k, max_ngram, drafts): shared with tests/test_gpu_spec_decode.py, which runs the draft kernel on them
DRAFT_CASES = [
    ([1, 2, 3, 4, 5], 3, 2, []),                                   # no match
    ([7, 1, 2, 8, 9, 2, 5, 6, 1, 2], 3, 2, [8, 9, 2]),             # ngram 2 (1 2 -> 8 9 2) wins over the ngram-1 matches of `2`
    ([4, 9, 9, 4, 1, 4, 2, 3, 4], 2, 2, [9, 9]),                   # no 2-gram (3 4) match; `4` matches at 0, 3, 5: the earliest wins
    ([3, 3], 4, 2, [3]),                                           # ngram 1: window 0 matches, its continuation is the last id
    ([5, 6, 7, 5, 6], 3, 1, [7, 5, 6]),                            # ngram 1 on `6`: index 1 -> 7 5 6; the match at the end (index 4) is the tail, skipped
    ([1, 2, 3, 1, 2], 8, 2, [3, 1, 2]),                            # continuation cut at the end of the history
    ([1, 2, 3, 4, 5, 6, 1, 2], 2, 2, [3, 4]),                      # continuation cut at k
    ([5], 3, 2, []),                                               # a history of one id
    ([8, 8, 8], 2, 9, [8]),                                        # max_ngram larger than the history: starts at len - 1 = 2 (8 8 at 0 -> [8])
]


@pytest.mark.parametrize("ids,k,max_ngram,want", DRAFT_CASES)
def test_prompt_lookup_draft_cases(ids, k, max_ngram, want):
    assert prompt_lookup_draft(ids, k, max_ngram) == want
    assert prompt_lookup_draft(torch.tensor(ids), k, max_ngram) == want


def test_prompt_lookup_draft_skips_a_match_without_continuation_for_a_smaller_ngram():
    # the only 2-gram window equal to the tail (2 2) that is not the tail itself is at index 1, whose continuation is the last id
    assert prompt_lookup_draft([1, 2, 2, 2], 3, 2) == [2]
    # nothing but the tail matches at any size
    assert prompt_lookup_draft([1, 2, 3], 3, 2) == []


def accept(a, token, n_draft):
    """The accept stage as include/vila_hip.h states it: a[i] the greedy pick of row i, token[1..] the drafts -> (m, appended ids, next token[0])."""
    a, token = np.asarray(a), np.asarray(token)
    m = 0
    while m < n_draft and a[m] == token[m + 1]:
        m += 1
    return m, a[:m + 1].tolist(), int(a[m])


@pytest.mark.parametrize("a,token,n_draft,want", [
    ([9, 4, 4, 4], [1, 4, 4, 4], 0, (0, [9], 9)),                  # no drafts: one token, whatever the padding rows say
    ([5, 6, 7, 8], [1, 5, 6, 7], 3, (3, [5, 6, 7, 8], 8)),         # all accepted: k drafts + the bonus token
    ([5, 6, 0, 8], [1, 5, 6, 7], 3, (2, [5, 6, 0], 0)),            # first mismatch at j = 2: the row's own pick replaces the draft
    ([3, 6, 7, 8], [1, 5, 6, 7], 3, (0, [3], 3)),                  # first mismatch at j = 0
    ([5, 6, 7, 8], [1, 5, 6, 7], 1, (1, [5, 6], 6)),               # padding rows ignored even where they would match
])
def test_accept_rule(a, token, n_draft, want):
    assert accept(a, token, n_draft) == want


NEW = ["vila_llm_decode_verify_workspace_bytes", "vila_llm_decode_step_verify", "vila_llm_decode_step_verify_w4", "vila_prompt_lookup_draft",
       "vila_attn_decode_verify_workspace_bytes", "vila_attn_decode_verify_bf16"]


def test_new_prototypes_on_both_sides():
    header = open(os.path.join(ROOT, "include", "vila_hip.h")).read()
    flat = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    for name in NEW:
        assert name in _lib.PROTOTYPES, name
        m = re.search(r"\b" + name + r"\s*\(([^;]*)\)\s*;", flat)
        assert m, f"{name} is not declared in include/vila_hip.h"
        n_args = 0 if m.group(1).strip() in ("", "void") else m.group(1).count(",") + 1
        assert n_args == len(_lib.PROTOTYPES[name][1]), f"{name}: {n_args} arguments in the header, {len(_lib.PROTOTYPES[name][1])} in _lib.PROTOTYPES"


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_decode_verify_layout_matches_the_header(tmp_path):
    cls = _lib.VilaDecodeVerify
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "vila_hip.h"', "int main(void) {",
             '    printf("sizeof %zu\\n", sizeof(VilaDecodeVerify));']
    lines += [f'    printf("{f[0]} %zu\\n", offsetof(VilaDecodeVerify, {f[0]}));' for f in cls._fields_]
    lines += ["    return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["sizeof"]) == C.sizeof(cls)
    assert [f[0] for f in cls._fields_] == ["n", "slot", "pos", "token", "n_draft", "out_ids", "n_out", "max_out", "logits", "n_accept", "hist", "n_hist",
                                            "hist_cap", "max_ngram", "cand", "n_cand"]
    for f in cls._fields_:
        assert int(got[f[0]]) == getattr(cls, f[0]).offset, f[0]


@pytest.fixture(scope="module")
def cpu_llm():
    from vila_amd.vlm import HipLlavaLlamaModel
    return HipLlavaLlamaModel(configs.tiny("mlp_downsample"), device="cpu").llm


def test_generate_refuses_what_the_mode_does_not_serve(cpu_llm):
    H = cpu_llm.lcfg.hidden_size
    one, two = torch.zeros(1, 4, H, dtype=torch.bfloat16), torch.zeros(2, 4, H, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="do_sample"):
        cpu_llm.generate(inputs_embeds=one, max_new_tokens=4, prompt_lookup_num_tokens=3, do_sample=True)
    with pytest.raises(ValueError, match="do_sample"):
        cpu_llm.generate(inputs_embeds=one, max_new_tokens=4, draft_ids=torch.tensor([1, 2, 3]), do_sample=True)
    with pytest.raises(ValueError, match="batch size 1"):
        cpu_llm.generate(inputs_embeds=two, max_new_tokens=4, prompt_lookup_num_tokens=3)
    for k in (0, 16, -1):
        with pytest.raises(ValueError, match="1..15"):
            cpu_llm.generate(inputs_embeds=one, max_new_tokens=4, prompt_lookup_num_tokens=k)
    with pytest.raises(ValueError, match="forced_ids"):
        cpu_llm.generate(inputs_embeds=one, max_new_tokens=4, prompt_lookup_num_tokens=3, forced_ids=torch.tensor([1, 2]))
    with pytest.raises(ValueError, match="return_logits"):
        cpu_llm.generate(inputs_embeds=one, max_new_tokens=4, prompt_lookup_num_tokens=3, return_logits=True)
    from types import SimpleNamespace
    with pytest.raises(ValueError, match="1..15"):                  # HF's name is read from generation_config as well
        cpu_llm.generate(inputs_embeds=one, max_new_tokens=4, generation_config=SimpleNamespace(prompt_lookup_num_tokens=40))
