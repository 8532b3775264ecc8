"""N3: the build's own CLIP BPE tokenizer against the token ids captured from the reference's SimpleTokenizer
(ppt_amd/data/classnames.json, written by tests/golden/make_golden.py).  The public CLIP merge table is not shipped (1.3 MB);
the tests read tests/golden/bpe_merges_subset.txt.gz, the same table with every merge the strings below can use kept at its
line (so ranks and ids are the real ones) and the others replaced by pairs that never match (make_golden.py bpe)."""
import json
import os

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_VOCAB = os.path.join(ROOT, "tests", "golden", "bpe_merges_subset.txt.gz")


def _tokenizer():
    from ppt_amd import tokenizer as T
    return T.SimpleTokenizer(GOLDEN_VOCAB)


def test_byte_symbol_table_is_a_bijection_without_whitespace():
    from ppt_amd import tokenizer as T
    tab = T.byte_symbols()
    assert len(set(tab.values())) == 256
    assert not any(c.isspace() for c in tab.values())
    assert tab[ord("a")] == "a" and tab[ord(" ")] == chr(256 + 32) and tab[0] == chr(256)


def test_encode_matches_captured_reference_ids():
    tok = _tokenizer()
    tab = json.load(open(os.path.join(ROOT, "ppt_amd", "data", "classnames.json")))
    assert tok.encoder["<|startoftext|>"] == tab["sot"] and tok.encoder["<|endoftext|>"] == tab["eot"]
    assert tok.encode("X") == [tab["placeholder"]] and tok.encode(".") == [tab["period"]]
    for name, ids in tab["name_tokens"].items():
        assert tok.encode(name) == ids, name


def test_prompt_rows_match_the_fixture_path():
    """tokenizer("X X ... X name.") == the row tokenize_prompts builds from the fixture (ULIP_models.py:87-100)."""
    tok = _tokenizer()
    from ppt_amd.models.ULIP_models import dataset_classnames, tokenize_prompts
    for ds in ("modelnet40", "scanobjectnn", "shapenetpart"):
        names = dataset_classnames(ds)
        want, lens = tokenize_prompts(names, 32)
        got = tok([" ".join(["X"] * 32) + " " + n.replace("_", " ") + "." for n in names])
        assert torch.equal(got, want)
        assert lens == [len(tok.encode(n.replace("_", " "))) for n in names]


def test_cleaning_contractions_digits_and_round_trip():
    tok = _tokenizer()
    assert tok.encode("A  Photo\nof a CAT") == tok.encode("a photo of a cat")
    assert tok.encode("&amp;amp;") == tok.encode("&")
    ids = tok.encode("it's 42 tables, isn't it?")
    assert tok.decode(ids) == "it 's 4 2 tables , isn 't it ? "
    row = tok("a chair", context_length=8)
    assert row.tolist()[0] == 49406 and row.tolist()[3] == 49407 and row.tolist()[4:] == [0] * 4
    long = tok("chair " * 100, context_length=77)
    assert long.shape == (77,) and int(long[-1]) != 0


def test_unknown_class_names_fall_back_to_the_tokenizer():
    tok = _tokenizer()
    from ppt_amd.models import ULIP_models as M
    ids, lens = M.tokenize_prompts(["rocking_horse", "chair"], 4, bpe_path=tok_path())
    assert lens == [len(tok.encode("rocking horse")), 1]
    assert ids[0].tolist()[:5] == [49406, 343, 343, 343, 343]
    assert ids[0].tolist()[5:5 + lens[0]] == tok.encode("rocking horse")


def tok_path():
    return GOLDEN_VOCAB


def test_single_row_is_squeezed_whatever_the_container():
    """utils/tokenizer.py:161-163: one row comes back as [context_length], for a str and for a one-element list."""
    tok = _tokenizer()
    assert tok("a chair").shape == (77,)
    assert tok(["a chair"]).shape == (77,)
    assert tok(["a chair", "a table"]).shape == (2, 77)


def test_uncaptured_class_name_is_tokenised_as_a_whole_string(monkeypatch):
    """A class name outside the committed id table goes through the tokenizer as the reference does it
    (ULIP_models.py:95-100): the whole "X ... X name." string at once -- a name ending in punctuation merges with the
    period into ONE piece, so the row is not [name pieces] + [period]."""
    tok = _tokenizer()
    from ppt_amd.models import ULIP_models as M
    monkeypatch.setenv("PPT_BPE_VOCAB", GOLDEN_VOCAB)
    names = ["lamp (floor)", "zebra crossing"]
    ids, lens = M.tokenize_prompts(names, 4)
    for row, n_name, name in zip(ids, lens, names):
        want = tok("X X X X " + name + ".")
        assert torch.equal(row, want), name
        assert n_name == len(tok.encode(name))
    pieces = tok.encode("lamp (floor).")
    assert pieces[-1] != tok.encode(".")[0], "')' and '.' merge into one BPE piece: the case the fallback must get right"
