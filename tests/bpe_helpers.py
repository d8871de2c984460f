"""Shared by test_bpe_tokenizer_cpu.py and test_bpe_tokenizer_gpu.py: byte-level BPE tokenizers trained in-process (no
pretrained vocabulary is available offline) in the three configurations the device path covers, and the text set."""
import ctypes
import functools

import numpy as np

CONFIGS = ("roberta", "roberta_prefix", "modernbert")

WORDS = ("the of and to in is that for it as was with be by on not he this are or his from at which but have an had they "
         "you were their one all we can her has there been if more when will would who so no out up into do any what them "
         "great product works well love much best purchase ever made terrible waste money awful buy broke after day fine "
         "nothing special average okay neither good bad password reset login help support please account payment refund "
         "shipping order tracking number classifier adaptive prototype memory neural network embedding transformer attention "
         "playing played plays player unbelievable internationalization tokenization tokenizer don't it's we'll they've I'm "
         "you're he'd can't").split()


def _corpus():
    rng = np.random.default_rng(5)
    out = []
    for _ in range(400):
        ws = [str(rng.choice(WORDS)) for _ in range(int(rng.integers(3, 14)))]
        if rng.random() < 0.3:
            ws.append(str(int(rng.integers(0, 100000))))
        out.append(" ".join(ws) + str(rng.choice([".", "!", "?", "...", ", ok", " (sic)", ""])))
    return out


@functools.lru_cache(maxsize=None)
def build_tokenizer(kind):
    """transformers PreTrainedTokenizerFast over a freshly trained ByteLevel + BPE pipeline.
    roberta / roberta_prefix: <s> ... </s> through RobertaProcessing, pad id 1; roberta returns no token_type_ids (as
    RobertaTokenizerFast), roberta_prefix names them in model_input_names and so returns them;
    modernbert: NFC normalizer, TemplateProcessing [CLS] $A [SEP], one added non-special token of two spaces."""
    from tokenizers import Tokenizer, models, normalizers, pre_tokenizers, processors, trainers, decoders
    from transformers import PreTrainedTokenizerFast
    assert kind in CONFIGS
    roberta = kind != "modernbert"
    specials = ["<s>", "<pad>", "</s>", "<unk>", "<mask>"] if roberta else ["[UNK]", "[CLS]", "[SEP]", "[PAD]", "[MASK]"]
    tk = Tokenizer(models.BPE())
    tk.pre_tokenizer = pre_tokenizers.ByteLevel(add_prefix_space=(kind == "roberta_prefix"), use_regex=True)
    tk.decoder = decoders.ByteLevel()
    if not roberta:
        tk.normalizer = normalizers.NFC()
    trainer = trainers.BpeTrainer(vocab_size=700, initial_alphabet=pre_tokenizers.ByteLevel.alphabet(), special_tokens=specials,
                                  show_progress=False)
    tk.train_from_iterator(_corpus(), trainer)
    if roberta:
        tk.post_processor = processors.RobertaProcessing(sep=("</s>", 2), cls=("<s>", 0))
        hf = PreTrainedTokenizerFast(tokenizer_object=tk, bos_token="<s>", eos_token="</s>", cls_token="<s>", sep_token="</s>",
                                     pad_token="<pad>", unk_token="<unk>", mask_token="<mask>",
                                     model_input_names=["input_ids", "attention_mask"] if kind == "roberta" else
                                     ["input_ids", "token_type_ids", "attention_mask"])
        assert hf.pad_token_id == 1
    else:
        tk.post_processor = processors.TemplateProcessing(single="[CLS] $A [SEP]", special_tokens=[("[CLS]", 1), ("[SEP]", 2)])
        hf = PreTrainedTokenizerFast(tokenizer_object=tk, cls_token="[CLS]", sep_token="[SEP]", pad_token="[PAD]",
                                     unk_token="[UNK]", mask_token="[MASK]")
        hf.add_tokens(["  "])
    return hf


FIXED = ["", " ", "  ", "a ", " a", "a   b  ",
         "\n's", " 's", "  's", "x''s", "'sabc", "'ss's", "x'rex", "it'S IT'S", "'ll'll 'lll", "1's 1'st",
         "a\tb\nc\rd\x0be\x0cf",
         "ctrl\x01in\x7fw \x00 nul \x1c\x1d\x1e\x1f x",
         "12345678901234567890", "a1b2c3",
         "x" * 300, "q" * 4096,
         "tail\n\n", "\n\n lead",
         "!@#$%^&*()_+-=[]{}|;':\",./<>?`~ ... ?!?! (a)[b]{c} 'd' \"e\" #tag @home $12.50 3%",
         "Hello, World!  This is GREAT...", "we'll see; they've gone, I'm sure you're right & he'd know"]


def host_route_texts(kind):
    """Texts the wrapper must hand to the wrapped tokenizer: non-ASCII, an emoji, a literal special token, over 4096 bytes."""
    special = "</s>" if kind != "modernbert" else "[SEP]"
    return ["café naïve résumé", "emoji \U0001f600 here", "has a %s literal inside" % special, "long " * 900]


def random_texts(n, seed):
    """Half word salads (case changes, digits, contractions, mixed separators), half random strings over a small alphabet
    rich in ' \\t\\n and the contraction letters or over all 128 ASCII bytes."""
    rng = np.random.default_rng(seed)
    small = list("' \t\nstmdrevlSTx1!") + ["  ", "'s", "'ll", " '"]
    out = []
    for i in range(n):
        if i % 2 == 0:
            ws = []
            for _ in range(int(rng.integers(1, 30))):
                w = str(rng.choice(WORDS))
                r = rng.random()
                if r < 0.15: w = w.upper()
                elif r < 0.3: w = w.capitalize()
                elif r < 0.4: w = w + str(int(rng.integers(0, 1000)))
                elif r < 0.5: w = w + str(rng.choice(list(",.;:!?'\"-()")))
                elif r < 0.6: w = w + str(rng.choice(["'s", "'t", "'re", "'ve", "'m", "'ll", "'d", "'S", "'x"]))
                elif r < 0.65: w = "".join(rng.choice(list("abcdefghijklmnopqrstuvwxyz"), int(rng.integers(1, 15))))
                ws.append(w)
            seps = [" ", " ", " ", "  ", "\t", "\n", " \n", "\n ", "   ", ""]
            out.append("".join(w + str(rng.choice(seps)) for w in ws))
        elif i % 4 == 1:
            out.append("".join(str(rng.choice(small)) for _ in range(int(rng.integers(1, 40)))))
        else:
            out.append(bytes(rng.integers(0, 128, int(rng.integers(1, 60))).astype(np.uint8)).decode("ascii"))
    return out


def text_set(kind, n_random, seed=11):
    return FIXED + host_route_texts(kind) + random_texts(n_random, seed)


def longest_pretoken(hf, text):
    """Bytes of the longest pre-token of an ASCII text (prefix space included), by the tokenizers library itself: ByteLevel
    writes one character per byte."""
    return max((len(piece) for piece, _ in hf.backend_tokenizer.pre_tokenizer.pre_tokenize_str(text)), default=0)


class HostVocab:
    """ac_bpe_vocab over host (numpy) arrays, built by the wrapper's own table builder."""

    def __init__(self, hf):
        from adaptive_classifier import tokenizer as tkz
        self.spec = tkz._bpe_spec(hf)
        assert self.spec is not None
        keys, entries, blob, byte_id, self.slots = tkz.build_bpe_tables(self.spec)
        self.arrays = (keys, entries, blob, byte_id)
        self.struct = tkz.bpe_vocab_struct(self.spec, [a.ctypes.data for a in self.arrays], self.slots)


def pack(texts):
    """(blob uint8 with 64 bytes of slack, offsets int32 [b + 1]) of ASCII texts"""
    raws = [t.encode("ascii") for t in texts]
    offs = np.zeros(len(raws) + 1, np.int32)
    offs[1:] = np.cumsum([len(r) for r in raws])
    blob = np.frombuffer(b"".join(raws) + b"\0" * 64, np.uint8).copy()
    return blob, offs


def dump(hv, texts, max_length, path):
    """Table + texts as one little-endian binary file, for a stand-alone C++ program over csrc/bpe_core.h:
    int32 [10] slots, blob bytes, b, text bytes, max_length, cls, sep, pad, add_prefix_space, 0 | keys | entries | blob |
    byte_id | offsets [b + 1] | text"""
    keys, entries, blob, byte_id = hv.arrays
    text, offs = pack(texts)
    text = text[:offs[-1]]                                 # exactly the texts' bytes: no slack behind the last one
    s = hv.spec
    head = np.array([hv.slots, len(blob), len(texts), len(text), max_length, s["cls_id"], s["sep_id"], s["pad_id"],
                     1 if s["add_prefix_space"] else 0, 0], np.int32)
    with open(path, "wb") as f:
        for a in (head, keys, entries, blob, byte_id, offs, text):
            f.write(np.ascontiguousarray(a).tobytes())


def encode_host(hv, texts, max_length):
    """ac_bpe_encode_host -> (ids int64 [b, max_length], mask, lens)"""
    from adaptive_classifier import _native as nv
    blob, offs = pack(texts)
    b = len(texts)
    ids = np.full((b, max_length), -7, np.int64)
    mask = np.full((b, max_length), -7, np.int64)
    lens = np.full(b, -7, np.int32)
    rc = nv.lib().ac_bpe_encode_host(blob.ctypes.data, offs.ctypes.data, b, ctypes.byref(hv.struct), max_length, ids.ctypes.data,
                                     mask.ctypes.data, lens.ctypes.data)
    assert rc == 0, nv.lib().ac_last_error()
    return ids, mask, lens
