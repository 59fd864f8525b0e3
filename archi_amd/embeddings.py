"""ArchiHipEmbeddings -- drop-in for the embedding provider the reference builds from
`data_manager.embedding_class_map[name]["class"](**kwargs)`
(/root/reference/src/data_manager/vectorstore/manager.py:66-73,
 src/archi/utils/vectorstore_connector.py:28-35, src/utils/config_service.py:470-496):
LangChain's `Embeddings` duck type with the constructor keywords of HuggingFaceEmbeddings
(src/cli/templates/base-config.yaml:143-150).

    embed_documents(texts: List[str]) -> List[List[float]]
    embed_query(text: str) -> List[float]

Errors are RAISED (never partial results): the manager records a failed file per exception
(manager.py:374-389).

Host side (this file): text normalisation, WordPiece tokenisation, length-sorted batching.
Device side: archi_amd.encoder.HipEncoder (hand-written HIP). No CPU fallback.
Qwen3-Embedding checkpoints (config.json model_type "qwen3") run on archi_amd.decoder.HipDecoder instead, tokenised by the
checkpoint's own tokenizer.json, pooled on the last token; ModernBERT checkpoints (model_type "modernbert") run on
archi_amd.modernbert.HipModernBert, NomicBERT checkpoints (model_type "nomic_bert") on archi_amd.nomic.HipNomicBert with the BERT
WordPiece tokenizer of their vocab.txt, Mistral / Llama checkpoints (model_type "mistral" | "llama") on archi_amd.llama.HipLlama, Qwen2 checkpoints
(model_type "qwen2") on archi_amd.qwen2.HipQwen2, T5 checkpoints (model_type "t5": gtr-t5, sentence-t5) on archi_amd.t5.HipT5; the same batching harness drives all of them.
"""
from __future__ import annotations

import ctypes
import os
import re
import threading
import zlib
from typing import Any, Callable, Dict, List, NamedTuple, Optional

import numpy as np

from . import _lib
from ._lib import check
from .encoder import (LONG_MAX_SEQ, MODEL_SHAPES, MPNET_SHAPES, XLMR_PADDING_IDX, XLMR_SHAPES, HipEncoder, load_hf_weights,
                      load_mpnet_weights, load_xlmr_weights, long_rows_supported, mpnet_rel_bias_table, random_init_weights,
                      random_mpnet_weights, random_xlmr_weights, read_sentence_transformers_config)
from .decoder import MAX_SEQ, QWEN3_SHAPES, BpeTokenizer, HipDecoder, load_qwen3_weights, random_qwen3_weights, read_decoder_st_config
from .modernbert import MODERNBERT_SHAPES, HipModernBert, load_modernbert_weights, random_modernbert_weights
from .modernbert import MAX_SEQ as MODERNBERT_MAX_SEQ
from .gemma import GEMMA_SHAPES, HipGemma, load_gemma_weights, random_gemma_weights
from .gemma import MAX_SEQ as GEMMA_MAX_SEQ
from .nomic import NOMIC_SHAPES, HipNomicBert, load_nomic_weights, nomic_config_info, random_nomic_weights
from .nomic import MAX_SEQ as NOMIC_MAX_SEQ
from .t5 import T5_SHAPES, HipT5, load_t5_weights, random_t5_weights
from .t5 import MAX_SEQ as T5_MAX_SEQ
from .llama import LLAMA_SHAPES, HipLlama, apply_mode, load_llama_weights, random_llama_weights, read_llama_st_config, resolve_mode
from .llama import MAX_SEQ as LLAMA_MAX_SEQ
from .qwen2 import QWEN2_SHAPES, HipQwen2, load_qwen2_weights, qwen2_config_shape, random_qwen2_weights
from .qwen2 import apply_mode as qwen2_apply_mode

CLS, SEP, PAD, UNK = 101, 102, 0, 100
# special tokens by name: (cls, sep, unk, the strings the full tokenizer matches in raw text)
BERT_SPECIALS = ("[CLS]", "[SEP]", "[UNK]", ("[CLS]", "[SEP]", "[UNK]", "[PAD]", "[MASK]"))
MPNET_SPECIALS = ("<s>", "</s>", "[UNK]", ("<s>", "</s>", "<pad>", "<mask>", "[UNK]"))      # transformers' MPNetTokenizer(Fast)


def _do_lower_case(model_dir: str) -> bool:
    """tokenizer_config.json's do_lower_case (BERT default: true), as the reference's AutoTokenizer reads it."""
    import json
    path = os.path.join(model_dir, "tokenizer_config.json")
    if os.path.exists(path):
        return bool(json.load(open(path)).get("do_lower_case", True))
    return True


class HashWordPiece:
    """Deterministic stand-in tokenizer for synthetic runs (no vocab.txt exists offline):
    lower-cased word/punctuation split, ids by CRC32 into [1000, vocab)."""

    def __init__(self, vocab: int = 30522):
        self.vocab = vocab
        self._re = re.compile(r"\w+|[^\w\s]")

    def encode(self, text: str, max_len: int) -> List[int]:
        ids = [CLS]
        for tok in self._re.findall(text.lower()):
            ids.append(1000 + zlib.crc32(tok.encode("utf-8")) % (self.vocab - 1000))
            if len(ids) >= max_len - 1:
                break
        ids.append(SEP)
        return ids

    def encode_batch(self, texts: List[str], max_len: int) -> List[List[int]]:
        return [self.encode(t, max_len) for t in texts]


class VocabWordPiece:
    """BERT WordPiece through the `tokenizers` wheel, from a local vocab.txt. specials: BERT_SPECIALS, or MPNET_SPECIALS for
    MPNet's <s> $A </s> post-processing with its own special tokens (as transformers' MPNetTokenizerFast builds it)."""

    def __init__(self, vocab_file: str, lowercase: bool = True, specials=BERT_SPECIALS):
        from tokenizers import BertWordPieceTokenizer
        cls, sep, unk, added = specials
        if specials == BERT_SPECIALS:
            self._tok = BertWordPieceTokenizer(vocab_file, lowercase=lowercase)
        else:
            from tokenizers.processors import TemplateProcessing
            self._tok = BertWordPieceTokenizer(vocab_file, lowercase=lowercase, unk_token=unk, sep_token=sep, cls_token=cls,
                                               pad_token=added[2], mask_token=added[3])
            self._tok.add_special_tokens(list(added))
            ci, si = self._tok.token_to_id(cls), self._tok.token_to_id(sep)
            self._tok.post_processor = TemplateProcessing(single=f"{cls} $A {sep}", special_tokens=[(cls, ci), (sep, si)])
        sep_id = self._tok.token_to_id(sep)
        self._sep = SEP if sep_id is None else sep_id

    def encode(self, text: str, max_len: int) -> List[int]:
        ids = self._tok.encode(text).ids
        if len(ids) > max_len:
            ids = ids[: max_len - 1] + [self._sep]
        return ids

    def encode_batch(self, texts: List[str], max_len: int) -> List[List[int]]:
        """One call into the Rust tokenizer for the whole list (it parallelises over its own thread pool), so
        ingestion-sized batches are not bound by a Python loop."""
        out = []
        for enc in self._tok.encode_batch(list(texts)):
            ids = enc.ids
            out.append(ids[: max_len - 1] + [self._sep] if len(ids) > max_len else ids)
        return out


class NativeWordPiece:
    """BERT WordPiece from a local vocab.txt through libarchi_hip.so's multi-threaded host tokenizer
    (ak_wordpiece_encode, csrc/wordpiece.cpp). Texts that need Unicode tables (any non-ASCII byte) or hold a literal
    special token come back flagged and go through the `tokenizers` wheel (VocabWordPiece), so the ids are always the
    reference tokenizer's."""

    def __init__(self, vocab_file: str, lowercase: bool = True, threads: int = 0, specials=BERT_SPECIALS):
        self._lib = _lib.load()
        h = ctypes.c_void_p()
        if specials == BERT_SPECIALS:
            check(self._lib.ak_wordpiece_create(vocab_file.encode(), int(lowercase), ctypes.byref(h)), "ak_wordpiece_create")
        else:                                # the model's own special tokens (MPNet): emitted and matched by name
            cls, sep, unk, added = specials
            arr = (ctypes.c_char_p * len(added))(*[a.encode() for a in added])
            check(self._lib.ak_wordpiece_create_ex(vocab_file.encode(), int(lowercase), cls.encode(), sep.encode(), unk.encode(),
                                                   arr, len(added), ctypes.byref(h)), "ak_wordpiece_create_ex")
        self._h = h
        self._threads = int(os.environ.get("ARCHI_TOKENIZER_THREADS", threads))
        self._vocab_file, self._lowercase, self._full, self._specials = vocab_file, lowercase, None, specials

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.ak_wordpiece_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _fallback(self) -> "VocabWordPiece":
        if self._full is None:
            self._full = VocabWordPiece(self._vocab_file, lowercase=self._lowercase, specials=self._specials)
        return self._full

    def encode_batch_array(self, texts: List[str], max_len: int):
        """-> (ids [n, max_len] int32 zero padded, lens [n] int32)."""
        n = len(texts)
        enc = [t.encode("utf-8", "surrogatepass") for t in texts]
        offs = np.zeros(n + 1, np.int64)
        np.cumsum(np.fromiter((len(e) for e in enc), np.int64, n), out=offs[1:])
        blob = b"".join(enc)
        ids = np.empty((n, max_len), np.int32)
        lens = np.empty(n, np.int32)
        check(self._lib.ak_wordpiece_encode(self._h, blob, offs.ctypes.data, n, max_len, self._threads,
                                            ids.ctypes.data, lens.ctypes.data), "ak_wordpiece_encode")
        rest = np.flatnonzero(lens < 0)
        if rest.size:
            for i, row in zip(rest, self._fallback().encode_batch([texts[i] for i in rest], max_len)):
                ids[i, : len(row)] = row
                lens[i] = len(row)
        return ids, lens

    def encode_batch(self, texts: List[str], max_len: int) -> List[List[int]]:
        ids, lens = self.encode_batch_array(texts, max_len)
        return [ids[i, : lens[i]].tolist() for i in range(len(texts))]

    def encode(self, text: str, max_len: int) -> List[int]:
        return self.encode_batch([text], max_len)[0]


def _is_qwen3(model_name: str) -> bool:
    """A Qwen3 checkpoint directory (config.json model_type "qwen3") or one of the named Qwen3-Embedding shapes."""
    import json
    if os.path.isdir(model_name):
        cj = os.path.join(model_name, "config.json")
        return os.path.exists(cj) and json.load(open(cj)).get("model_type") == "qwen3"
    return model_name in QWEN3_SHAPES


def _is_modernbert(model_name: str) -> bool:
    """A ModernBERT checkpoint directory (config.json model_type "modernbert") or one of the named ModernBERT shapes."""
    import json
    if os.path.isdir(model_name):
        cj = os.path.join(model_name, "config.json")
        return os.path.exists(cj) and json.load(open(cj)).get("model_type") == "modernbert"
    return model_name in MODERNBERT_SHAPES


def _is_gemma(model_name: str) -> bool:
    """An EmbeddingGemma checkpoint directory (config.json model_type "gemma3_text") or one of the named Gemma shapes."""
    import json
    if os.path.isdir(model_name):
        cj = os.path.join(model_name, "config.json")
        return os.path.exists(cj) and json.load(open(cj)).get("model_type") == "gemma3_text"
    return model_name in GEMMA_SHAPES


def _is_nomic(model_name: str) -> bool:
    """A NomicBERT checkpoint directory (config.json model_type "nomic_bert") or one of the named NomicBERT shapes."""
    import json
    if os.path.isdir(model_name):
        cj = os.path.join(model_name, "config.json")
        return os.path.exists(cj) and json.load(open(cj)).get("model_type") == "nomic_bert"
    return model_name in NOMIC_SHAPES


def _is_t5(model_name: str) -> bool:
    """A T5 checkpoint directory (config.json model_type "t5") or one of the named T5 shapes."""
    import json
    if os.path.isdir(model_name):
        cj = os.path.join(model_name, "config.json")
        return os.path.exists(cj) and json.load(open(cj)).get("model_type") == "t5"
    return model_name in T5_SHAPES


def _is_llama(model_name: str) -> bool:
    """A Mistral / Llama checkpoint directory (config.json model_type "mistral" | "llama") or one of the named shapes."""
    import json
    if os.path.isdir(model_name):
        cj = os.path.join(model_name, "config.json")
        return os.path.exists(cj) and json.load(open(cj)).get("model_type") in ("mistral", "llama")
    return model_name in LLAMA_SHAPES


def _is_qwen2(model_name: str) -> bool:
    """A Qwen2 checkpoint directory (config.json model_type "qwen2") or one of the named Qwen2 shapes."""
    import json
    if os.path.isdir(model_name):
        cj = os.path.join(model_name, "config.json")
        return os.path.exists(cj) and json.load(open(cj)).get("model_type") == "qwen2"
    return model_name in QWEN2_SHAPES


def _is_mpnet(model_name: str) -> bool:
    """An MPNet checkpoint directory (config.json model_type "mpnet") or one of the named MPNet shapes."""
    import json
    if os.path.isdir(model_name):
        cj = os.path.join(model_name, "config.json")
        return os.path.exists(cj) and json.load(open(cj)).get("model_type") == "mpnet"
    return model_name in MPNET_SHAPES


def _is_xlmr(model_name: str) -> bool:
    """An XLM-RoBERTa / RoBERTa checkpoint directory (config.json model_type "xlm-roberta" | "roberta") or a named XLM-R shape."""
    import json
    if os.path.isdir(model_name):
        cj = os.path.join(model_name, "config.json")
        return os.path.exists(cj) and json.load(open(cj)).get("model_type") in ("xlm-roberta", "roberta")
    return model_name in XLMR_SHAPES


# longest row of the parity modes (and of bf16 at head size 32 / hidden 384); bf16 at head size 64 runs up to LONG_MAX_SEQ
ENCODER_MAX_SEQ = 512


class _StackFamily(NamedTuple):
    """What ArchiHipEmbeddings._init_stack needs to know of a pre-norm stack family."""
    models: str                 # "<models> run in bf16 only"
    checkpoint: str             # with its article: "Pass <checkpoint> checkpoint directory"
    tokenizer: str              # "... checkpoint needs its <tokenizer>"
    shapes: Dict[str, tuple]    # named shapes (synthetic_seed)
    max_position: int           # index of max_position in a shape tuple (hidden is index 1 in all three)
    max_seq: int                # longest row the kernels take
    load: Callable              # checkpoint directory -> (shape, weights)
    st_config: Callable         # checkpoint directory -> (pooling, max_seq_length | None, always_normalise)
    random: Callable            # (shape, model_kwargs) -> seeded random weights
    pooling: Callable           # (model_name, shape, model_kwargs, the checkpoint's pooling | None) -> pooling
    handle: Callable            # the HipStack subclass
    wordpiece: bool = False     # a vocab.txt beside the weights (or model_kwargs["vocab_file"]) is the tokenizer: BERT WordPiece
    precheck: Optional[Callable] = None      # (checkpoint directory, model_kwargs): refusals the config alone decides, before any GPU work
    reshape: Optional[Callable] = None       # (shape, model_kwargs) -> the shape the handle is built from (a mode the caller states)


def _seed_std(kw):
    return dict(seed=int(kw["synthetic_seed"]), std=float(kw.get("synthetic_std", 0.02)))


def _gemma_pooling(model_name, shape, kw, st_pool):
    if st_pool is not None and kw.get("pooling", st_pool) != "mean":
        raise ValueError(f"{model_name}: pooling {kw.get('pooling', st_pool)!r} (Gemma embedders pool 'mean')")
    return "mean"


# Qwen3-Embedding: lasttoken pooling, rows up to 8192 tokens
_QWEN3 = _StackFamily("decoder models (Qwen3)", "a Qwen3", "byte-level BPE tokenizer", QWEN3_SHAPES, 6, MAX_SEQ, load_qwen3_weights,
                      lambda d: ("last",) + tuple(read_decoder_st_config(d)),
                      lambda shape, kw: random_qwen3_weights(shape, seed=int(kw["synthetic_seed"])),
                      lambda name, shape, kw, st_pool: "last", HipDecoder)
# ModernBERT (nomic-ai/modernbert-embed-base, Alibaba-NLP/gte-modernbert-base, lightonai/modernbert-embed-large): mean or cls pooling
# as the checkpoint or the named shape says, rows up to 8192 tokens
_MODERNBERT = _StackFamily("ModernBERT models", "a ModernBERT", "BPE tokenizer", MODERNBERT_SHAPES, 5, MODERNBERT_MAX_SEQ, load_modernbert_weights,
                           read_sentence_transformers_config, lambda shape, kw: random_modernbert_weights(shape, **_seed_std(kw)),
                           lambda name, shape, kw, st_pool: kw.get("pooling", st_pool or shape[11]), HipModernBert)
# EmbeddingGemma (google/embeddinggemma-300m; its tokenizer.json's post-processor adds <bos> / <eos>; the 2_Dense / 3_Dense modules
# come with the weights): mean pooling, rows up to 2048 tokens
_GEMMA = _StackFamily("Gemma embedders", "an EmbeddingGemma", "tokenizer", GEMMA_SHAPES, 7, GEMMA_MAX_SEQ, load_gemma_weights,
                      read_sentence_transformers_config, lambda shape, kw: random_gemma_weights(shape, **_seed_std(kw)), _gemma_pooling, HipGemma)


def _nomic_precheck(model_dir, kw):
    """A dynamic-NTK RoPE checkpoint equals the default RoPE up to its trained length and nothing computes it beyond: a larger
    explicit max_seq_length is refused, not truncated."""
    import json
    cj = os.path.join(model_dir, "config.json")
    shape, dynamic = nomic_config_info(json.load(open(cj)), cj)
    if dynamic and "max_seq_length" in kw and int(kw["max_seq_length"]) > shape[6]:
        raise ValueError(f"{model_dir}: max_seq_length {int(kw['max_seq_length'])} is past the trained length {shape[6]} of a dynamic-NTK "
                         f"RoPE checkpoint (rows up to {shape[6]} tokens equal the default RoPE; longer rows are not implemented)")


# NomicBERT (nomic-ai/nomic-embed-text-v1 / -v1.5 / -v1-unsupervised, Snowflake/snowflake-arctic-embed-m-long): mean or cls pooling as the
# checkpoint or the named shape says, rows up to 8192 tokens (a dynamic-NTK checkpoint: up to its trained length), BERT WordPiece
_NOMIC = _StackFamily("NomicBERT models", "a NomicBERT", "vocab.txt or tokenizer.json", NOMIC_SHAPES, 6, NOMIC_MAX_SEQ, load_nomic_weights,
                      read_sentence_transformers_config, lambda shape, kw: random_nomic_weights(shape, **_seed_std(kw)),
                      lambda name, shape, kw, st_pool: kw.get("pooling", st_pool or shape[9]), HipNomicBert, wordpiece=True,
                      precheck=_nomic_precheck)


def _t5_st_config(model_dir):
    """read_sentence_transformers_config, and the refusal of a pool that leaves the prompt's tokens out (instructor's 1_Pooling):
    prompts stay with the caller, so the pool cannot know how many tokens one holds."""
    import json
    pj = os.path.join(model_dir, "1_Pooling", "config.json")
    if os.path.exists(pj) and json.load(open(pj)).get("include_prompt", True) is False:
        raise ValueError(f"{pj}: include_prompt false is not supported (the pool would leave the prompt's tokens out, and prompts stay "
                         "with the caller: the provider cannot know their length)")
    return read_sentence_transformers_config(model_dir)


def _t5_random(shape, kw):
    return random_t5_weights(shape, seed=int(kw["synthetic_seed"]), std=float(kw.get("synthetic_std", 0.05)),
                             bias_std=float(kw.get("synthetic_bias_std", 2.0)))


# T5 encoders (sentence-transformers/gtr-t5-base / -large, sentence-t5-base / -large, instructor directories whose pool includes the
# prompt): mean or cls pooling as the checkpoint or the named shape says, the Dense modules come with the weights, rows up to 8192
# tokens (the model has no position limit); the checkpoint's own tokenizer.json (Unigram), whose post-processor appends </s>
_T5 = _StackFamily("T5 embedders", "a T5", "tokenizer.json (its post-processor appends </s>)", T5_SHAPES, 10, T5_MAX_SEQ, load_t5_weights,
                   _t5_st_config, _t5_random, lambda name, shape, kw, st_pool: kw.get("pooling", st_pool or shape[11]), HipT5,
                   precheck=lambda model_dir, kw: _t5_st_config(model_dir))


def _llama_precheck(model_dir, kw):
    """What the sentence-transformers files and the keywords alone decide (an attention mode or a pooling that does not exist), before
    the weights are read."""
    st_pool, _, _ = read_llama_st_config(model_dir)
    resolve_mode(model_dir, None, kw, st_pool)


# Mistral / Llama embedders (intfloat/e5-mistral-7b-instruct, Salesforce/SFR-Embedding-Mistral, Linq-AI-Research/Linq-Embed-Mistral, the
# Llama-3.1-8B based ones): causal attention with the config's sliding window and lasttoken pooling, or -- model_kwargs["attention"] =
# "bidirectional", the caller's statement of how the checkpoint was trained -- every key below the length and mean pooling
# (llama.resolve_mode; model_kwargs["pooling"] overrides); rows up to 8192 tokens; the special tokens are whatever the tokenizer.json's
# post-processor adds. LLAMA_SHAPES also names the small shapes of the test fixtures (synthetic_seed only), as the other families' do
_LLAMA = _StackFamily("Mistral / Llama embedders", "a Mistral or Llama", "tokenizer", LLAMA_SHAPES, 6, LLAMA_MAX_SEQ, load_llama_weights,
                      read_llama_st_config, lambda shape, kw: random_llama_weights(shape, **_seed_std(kw)), resolve_mode, HipLlama,
                      precheck=_llama_precheck, reshape=apply_mode)


def _qwen2_precheck(model_dir, kw):
    """What config.json, the sentence-transformers files and the keywords alone decide, before the weights are read."""
    import json
    cj = os.path.join(model_dir, "config.json")
    shape = qwen2_config_shape(json.load(open(cj)), cj)
    st_pool, _, _ = read_llama_st_config(model_dir)
    resolve_mode(model_dir, shape, kw, st_pool)


def _qwen2_random(shape, kw):
    return random_qwen2_weights(shape, bias_std=float(kw.get("synthetic_bias_std", 2.0)), **_seed_std(kw))


# Qwen2 / Qwen2.5 embedders (Alibaba-NLP/gte-Qwen2-1.5B-instruct and -7B-instruct, gte-Qwen1.5-7B-instruct, infly/inf-retriever-v1): q / k / v
# biases and up to 8 query heads per kv head; causal attention and lasttoken pooling unless config.json says is_causal: false or
# model_kwargs["attention"] = "bidirectional" (the keyword wins; llama.resolve_mode, model_kwargs["pooling"] overrides); rows up to 8192
# tokens; prompts and special tokens stay with the caller and the tokenizer.json's post-processor, as for the Llama family
_QWEN2 = _StackFamily("Qwen2 embedders", "a Qwen2", "byte-level BPE tokenizer", QWEN2_SHAPES, 6, LLAMA_MAX_SEQ, load_qwen2_weights,
                      read_llama_st_config, _qwen2_random, resolve_mode, HipQwen2, precheck=_qwen2_precheck, reshape=qwen2_apply_mode)


class ArchiHipEmbeddings:
    def __init__(self, model_name: str = "sentence-transformers/all-MiniLM-L6-v2",
                 model_kwargs: Optional[Dict[str, Any]] = None, encode_kwargs: Optional[Dict[str, Any]] = None,
                 **_ignored: Any):
        """model_name: a known architecture name or a local HF checkpoint directory.
        model_kwargs: {"device": "cuda[:i]"} ; {"synthetic_seed": int} builds seeded random-init weights of the
        named architecture (benchmarks/tests: the image has no checkpoints and no network); {"residual": "f32"} keeps
        the residual stream between layers in fp32 (default "bf16", see HipEncoder); {"precision": "f32"} selects the
        float32 parity mode (float32 weights and arithmetic, ~1e-6 from the reference's CPU embedder, ~1/9 of the bf16 rate),
        {"precision": "bf16x3"} the split-bf16 parity mode (float32 weights, GEMMs as three bf16 MFMA passes into one float32
        accumulator: the same top-k and scores within 1e-5 of the CPU path at ~3x the "f32" mode's rate).
        encode_kwargs: {"normalize_embeddings": bool, "batch_tokens": int}."""
        self.model_name = model_name
        self.model_kwargs = dict(model_kwargs or {})
        self.encode_kwargs = dict(encode_kwargs or {})
        self.normalize = bool(self.encode_kwargs.get("normalize_embeddings", False))
        self.batch_tokens = int(self.encode_kwargs.get("batch_tokens", 65536))
        dev = str(self.model_kwargs.get("device", "cuda"))
        device = int(dev.split(":")[1]) if ":" in dev else None
        self._stage = self._stage_out = None
        self._stage_lock = threading.Lock()
        for is_family, family in ((_is_qwen3, _QWEN3), (_is_modernbert, _MODERNBERT), (_is_gemma, _GEMMA), (_is_nomic, _NOMIC),
                                  (_is_llama, _LLAMA), (_is_qwen2, _QWEN2), (_is_t5, _T5)):
            if is_family(model_name):
                self._init_stack(family, model_name, device)
                return
        rel_bias = pos_pad = None
        if _is_xlmr(model_name):
            vocab, H, L, heads, I, max_pos, weights, eps, pos_pad = self._init_xlmr(model_name)
        elif _is_mpnet(model_name):
            vocab, H, L, heads, I, max_pos, weights, eps, rel_bias = self._init_mpnet(model_name)
        elif os.path.isdir(model_name):
            shape, weights, eps = load_hf_weights(model_name)
            vocab, H, L, heads, I, max_pos = shape
            st_pool, st_len, st_norm = read_sentence_transformers_config(model_name)
            self.pooling = self.model_kwargs.get("pooling", st_pool)
            self.max_seq_length = min(int(self.model_kwargs.get("max_seq_length", st_len or max_pos)), max_pos, 512)
            self.normalize = self.normalize or st_norm     # a Normalize module in the checkpoint always applies
            vf, tf = os.path.join(model_name, "vocab.txt"), os.path.join(model_name, "tokenizer.json")
            if os.path.exists(vf):
                self.tokenizer = NativeWordPiece(vf, lowercase=_do_lower_case(model_name))
            elif os.path.exists(tf):
                # BERT weights with an XLM-R tokenizer and no vocab.txt (paraphrase-multilingual-MiniLM-L12-v2,
                # multilingual-e5-small): the checkpoint's own tokenizer.json, as AutoTokenizer would load it
                self.tokenizer = BpeTokenizer(tf)
            else:
                # real weights + hashed token ids = garbage embeddings with no error. The reference's embedder
                # (HuggingFaceEmbeddings -> SentenceTransformer -> AutoTokenizer [upstream]) raises when the checkpoint
                # has no tokenizer; HashWordPiece is only for seeded random-init models (synthetic_seed).
                raise FileNotFoundError(f"{model_name}: neither vocab.txt nor tokenizer.json found -- a checkpoint directory needs "
                                        "its tokenizer (the hashing stand-in tokenizer is only used with synthetic_seed)")
        elif model_name in MODEL_SHAPES and "synthetic_seed" in self.model_kwargs:
            vocab, H, L, heads, I, max_pos, self.pooling, self.max_seq_length = MODEL_SHAPES[model_name]
            weights = random_init_weights(vocab, H, L, I, max_pos, seed=int(self.model_kwargs["synthetic_seed"]))
            eps = 1e-12
            vf = self.model_kwargs.get("vocab_file")          # benchmarks: a synthetic vocab.txt for the random-init model
            self.tokenizer = NativeWordPiece(vf) if vf else HashWordPiece(vocab)
        else:
            raise FileNotFoundError(
                f"{model_name!r}: no local checkpoint directory (offline image). Pass a directory with config.json + "
                "model.safetensors (+ vocab.txt), or model_kwargs={'synthetic_seed': N} for seeded random weights")
        self.dimensions = H
        self.encoder = HipEncoder(vocab, H, L, heads, I, max_pos, weights, ln_eps=eps, device=device,
                                  residual=str(self.model_kwargs.get("residual", "bf16")),
                                  precision=str(self.model_kwargs.get("precision", "bf16")), rel_bias=rel_bias,
                                  positions_from_ids=pos_pad)

    def _init_xlmr(self, model_name: str):
        """XLM-RoBERTa (bge-m3, multilingual-e5, paraphrase-multilingual-mpnet-base-v2): a local checkpoint directory (config.json
        model_type xlm-roberta | roberta, safetensors, tokenizer.json, the sentence-transformers files) or a named shape with
        synthetic_seed. The BERT encoder with positions from the ids (ak_encoder_set_positions_from_ids), the model's token-type row
        and its tokenizer.json; every precision. Rows up to 8192 tokens in bf16 at head size 64 (csrc/attn_long.hip), 512 otherwise:
        a max_seq_length above that is refused before any GPU work (the provider never truncates silently)."""
        precision = str(self.model_kwargs.get("precision", "bf16"))
        if os.path.isdir(model_name):
            import json
            cfg = json.load(open(os.path.join(model_name, "config.json")))
            hidden, heads = int(cfg.get("hidden_size", 0)), int(cfg.get("num_attention_heads", 1))
            pad = int(cfg.get("pad_token_id", XLMR_PADDING_IDX))
            usable = int(cfg.get("max_position_embeddings", 514)) - pad - 1
            st_pool, st_len, st_norm = read_sentence_transformers_config(model_name)
            self.pooling = self.model_kwargs.get("pooling", st_pool)
            self.normalize = self.normalize or st_norm
        elif "synthetic_seed" in self.model_kwargs:
            shape = XLMR_SHAPES[model_name]
            hidden, heads = shape[1], shape[3]
            pad, usable = XLMR_PADDING_IDX, shape[5] - XLMR_PADDING_IDX - 1
            st_len = shape[7]
            self.pooling = self.model_kwargs.get("pooling", shape[6])
            self.normalize = True                      # the released sentence-transformers models carry a Normalize module
        else:
            raise FileNotFoundError(f"{model_name!r}: no local checkpoint directory (offline image). Pass an XLM-RoBERTa checkpoint "
                                    "directory, or model_kwargs={'synthetic_seed': N} for seeded random weights")
        self.max_seq_length = min(int(self.model_kwargs.get("max_seq_length", st_len or usable)), usable, LONG_MAX_SEQ)
        if self.max_seq_length > ENCODER_MAX_SEQ and not long_rows_supported(hidden, heads, precision):
            raise ValueError(f"{model_name}: max_seq_length {self.max_seq_length} -- rows longer than {ENCODER_MAX_SEQ} tokens run in "
                             f"precision 'bf16' at head size 64 only (here precision {precision!r}, head size {hidden / heads:g}); pass "
                             f"model_kwargs={{'max_seq_length': {ENCODER_MAX_SEQ}}} to truncate chunks at {ENCODER_MAX_SEQ} tokens")
        if os.path.isdir(model_name):
            shape, weights, eps, pad = load_xlmr_weights(model_name)
            vocab, H, L, heads, I, max_pos = shape
            tf = os.path.join(model_name, "tokenizer.json")
            if not os.path.exists(tf):
                raise FileNotFoundError(f"{model_name}: tokenizer.json not found -- an XLM-RoBERTa checkpoint needs its tokenizer")
            self.tokenizer = BpeTokenizer(tf)
        else:
            vocab, H, L, heads, I, max_pos = shape[:6]
            weights = random_xlmr_weights(shape, seed=int(self.model_kwargs["synthetic_seed"]))
            eps = 1e-5
            tf = self.model_kwargs.get("tokenizer_file")
            self.tokenizer = BpeTokenizer(tf) if tf else HashWordPiece(vocab)
        return vocab, H, L, heads, I, max_pos, weights, eps, pad

    def _init_mpnet(self, model_name: str):
        """MPNet (all-mpnet-base-v2 and its family): a local checkpoint directory (config.json model_type mpnet, safetensors,
        vocab.txt, the sentence-transformers files) or a named shape with synthetic_seed. The BERT encoder with MPNet's
        relative-position bias, its offset positions and its <s> ... </s> tokenizer; every precision."""
        if os.path.isdir(model_name):
            shape, weights, rel_w, eps = load_mpnet_weights(model_name)
            vocab, H, L, heads, I, max_pos = shape
            st_pool, st_len, st_norm = read_sentence_transformers_config(model_name)
            self.pooling = self.model_kwargs.get("pooling", st_pool)
            self.max_seq_length = min(int(self.model_kwargs.get("max_seq_length", st_len or max_pos)), max_pos, 512)
            self.normalize = self.normalize or st_norm
            vf = os.path.join(model_name, "vocab.txt")
            if not os.path.exists(vf):
                raise FileNotFoundError(f"{model_name}: vocab.txt not found -- an MPNet checkpoint directory needs its WordPiece "
                                        "vocabulary (the hashing stand-in tokenizer is only used with synthetic_seed)")
            self.tokenizer = NativeWordPiece(vf, lowercase=_do_lower_case(model_name), specials=MPNET_SPECIALS)
        elif "synthetic_seed" in self.model_kwargs:
            shape = MPNET_SHAPES[model_name]
            vocab, H, L, heads, I = shape[:5]
            max_pos = min(shape[5] - 2, 512)
            self.pooling, self.max_seq_length = shape[6], min(shape[7], max_pos)
            weights, rel_w, _ = random_mpnet_weights(shape, seed=int(self.model_kwargs["synthetic_seed"]))
            eps = 1e-5
            self.normalize = True                      # the released sentence-transformers models carry a Normalize module
            vf = self.model_kwargs.get("vocab_file")
            self.tokenizer = NativeWordPiece(vf, specials=MPNET_SPECIALS) if vf else HashWordPiece(vocab)
        else:
            raise FileNotFoundError(f"{model_name!r}: no local checkpoint directory (offline image). Pass an MPNet checkpoint "
                                    "directory, or model_kwargs={'synthetic_seed': N} for seeded random weights")
        return vocab, H, L, heads, I, max_pos, weights, eps, mpnet_rel_bias_table(rel_w, max_pos)

    def _init_stack(self, fam: "_StackFamily", model_name: str, device: Optional[int]) -> None:
        """A stack family (Qwen3-Embedding, ModernBERT, EmbeddingGemma, NomicBERT; the _StackFamily records above): a local checkpoint
        directory (config.json of the family's model_type, safetensors, tokenizer.json -- NomicBERT: vocab.txt first --, the
        sentence-transformers files) or a named shape with synthetic_seed. bf16 only. Query / document prompts stay with the caller, as the reference's retrievers handle
        instructions themselves."""
        precision = str(self.model_kwargs.get("precision", "bf16"))
        if precision != "bf16":
            raise ValueError(f"precision {precision!r}: {fam.models} run in bf16 only")
        if os.path.isdir(model_name):
            tf, vf = os.path.join(model_name, "tokenizer.json"), os.path.join(model_name, "vocab.txt")
            use_vocab = fam.wordpiece and os.path.exists(vf)
            if not use_vocab and not os.path.exists(tf):
                raise FileNotFoundError(f"{model_name}: tokenizer.json not found -- {fam.checkpoint} checkpoint needs its {fam.tokenizer}")
            if fam.precheck:
                fam.precheck(model_name, self.model_kwargs)
            shape, weights = fam.load(model_name)
            st_pool, st_len, st_norm = fam.st_config(model_name)
            self.normalize = self.normalize or st_norm
            self.tokenizer = NativeWordPiece(vf, lowercase=_do_lower_case(model_name)) if use_vocab else BpeTokenizer(tf)
        else:
            if "synthetic_seed" not in self.model_kwargs:
                raise FileNotFoundError(f"{model_name!r}: no local checkpoint directory (offline image). Pass {fam.checkpoint} checkpoint "
                                        "directory, or model_kwargs={'synthetic_seed': N} for seeded random weights")
            shape = fam.shapes[model_name]
            weights = fam.random(shape, self.model_kwargs)
            st_pool, st_len = None, None
            self.normalize = True                      # the released sentence-transformers models carry a Normalize module
            tf, vf = self.model_kwargs.get("tokenizer_file"), self.model_kwargs.get("vocab_file") if fam.wordpiece else None
            self.tokenizer = NativeWordPiece(vf) if vf else BpeTokenizer(tf) if tf else HashWordPiece(shape[0])
        self.pooling = fam.pooling(model_name, shape, self.model_kwargs, st_pool)
        max_pos = int(shape[fam.max_position])
        self.max_seq_length = min(int(self.model_kwargs.get("max_seq_length", st_len or max_pos)), max_pos, fam.max_seq)
        if fam.reshape:
            shape = fam.reshape(shape, self.model_kwargs)
        self.encoder = fam.handle(shape, weights, device=device)
        self.dimensions = int(self.encoder.out_dim)

    # -- LangChain Embeddings duck type -------------------------------------
    def embed_documents(self, texts: List[str]) -> List[List[float]]:
        return self.embed_documents_array(texts).tolist()   # float32 values widened to Python floats (a1)

    def embed_documents_array(self, texts: List[str]) -> np.ndarray:
        """embed_documents without the List[List[float]] conversion (which costs more than the GPU work at ingestion
        sizes): the build's own callers (ArchiHipVectorStore.add_texts, BatchedIngestor) take the float32 rows."""
        texts = [t.replace("\n", " ") for t in texts]       # langchain_huggingface does the same [upstream]
        if not texts:
            return np.empty((0, self.dimensions), np.float32)
        if hasattr(self.tokenizer, "encode_batch_array"):
            return self.embed_token_arrays(*self.tokenizer.encode_batch_array(texts, self.max_seq_length))
        return self.embed_token_lists(self.tokenizer.encode_batch(texts, self.max_seq_length))

    def embed_query(self, text: str) -> List[float]:
        return self.embed_documents([text])[0]

    # -- batching harness (the build's counterpart of manager.py:362-373: cross-file, length-sorted) --
    def embed_token_lists(self, toks: List[List[int]]) -> np.ndarray:
        """Token lists -> embeddings (see embed_token_arrays)."""
        import itertools
        n = len(toks)
        lens = np.fromiter((len(t) for t in toks), np.int32, n)
        width = max(1, int(lens.max())) if n else 1
        ids = np.zeros((n, width), np.int32)
        if n:
            ids[np.arange(width)[None, :] < lens[:, None]] = np.fromiter(itertools.chain.from_iterable(toks), np.int32,
                                                                         int(lens.sum()))
        return self.embed_token_arrays(ids, lens)

    def embed_token_arrays(self, ids: np.ndarray, lens: np.ndarray) -> np.ndarray:
        """ids [n, W] int32 (row i holds lens[i] ids, zero padded) -> [n, D] float32.
        Length-sorted [B,S] tiles (S a multiple of 32, about `batch_tokens` tokens per tile). Per tile the host only
        gathers the tile's rows into a pinned buffer (one asynchronous copy); the mask is laid out on the device, every
        forward pass is enqueued without waiting for the previous one, and the embeddings come back in ONE
        device-to-host copy at the end -- the host prepares tile i+1 while the GPU runs tile i."""
        import torch
        n = len(lens)
        out = np.empty((n, self.dimensions), dtype=np.float32)
        if n == 0:
            return out
        lens = np.asarray(lens, np.int64)
        order = np.argsort(-lens, kind="stable")
        dev = getattr(self.encoder, "_dev", None)
        on_gpu = dev is not None and dev.type == "cuda"
        # tile plan first: (start, rows, S) and the staging offset of each tile ([rows, S + 1] int32, column S = length)
        plan, need, i = [], 0, 0
        while i < n:
            S = max(32, (int(lens[order[i]]) + 31) // 32 * 32)
            nb = min(max(1, self.batch_tokens // S), n - i)
            plan.append((i, nb, S, need))
            need += nb * (S + 1)
            i += nb
        with self._stage_lock:
            # ONE pinned staging area per provider, grow-only and reused across calls (a call ends with a full
            # synchronisation, so nothing of it is in flight when the next one starts): a pinned allocation per tile made
            # the caching host allocator fall back to hipHostMalloc whenever the previous tiles' copies were still in
            # flight -- identical calls took 39 to 95 ms
            if self._stage is None or self._stage.numel() < need:
                self._stage = torch.empty(max(need, 1 << 20), dtype=torch.int32, pin_memory=on_gpu)
            if self._stage_out is None or self._stage_out.numel() < n * self.dimensions:
                self._stage_out = torch.empty(max(n * self.dimensions, 1 << 20), dtype=torch.float32, pin_memory=on_gpu)
            host = self._stage.numpy()
            parts = []
            lens_path = on_gpu and hasattr(self.encoder, "forward_lens")
            dev_out = torch.empty((n, self.dimensions), dtype=torch.float32, device=dev) if lens_path else None
            for start, nb, S, off in plan:
                chunk = order[start: start + nb]
                view = host[off: off + nb * (S + 1)].reshape(nb, S + 1)
                w = min(S, ids.shape[1])
                # rows first, columns second: np.take on the column-sliced (strided) view with a strided `out` copied the WHOLE
                # id matrix once per tile -- quadratic in the call size (81k chunks: 2.5 s instead of 0.6). Measured with this
                # fixed and not kept: tokenising slice i + 1 on a host thread while the GPU embeds slice i (8k / 16k / 32k
                # texts per slice: 129 / 127 / 130 k chunks/s against 131 k for the one pass -- a sync and a D2H per slice
                # cost what the hidden tokeniser time, a tenth of the call, would have saved)
                view[:, :w] = ids[chunk, :w] if w == ids.shape[1] else ids[chunk][:, :w]
                if w < S:
                    view[:, w:S] = 0
                view[:, S] = lens[chunk]
                stage = self._stage[off: off + nb * (S + 1)].view(nb, S + 1)
                if lens_path:
                    # ONE asynchronous copy per tile, then the library: it lays the mask out from the lengths and writes the
                    # tile's rows at their place in the call's result buffer (no torch kernel between the H2D and the final D2H)
                    self.encoder.forward_lens(stage.to(dev, non_blocking=True), nb, S, dev_out[start: start + nb],
                                              pooling=self.pooling, normalise=self.normalize)
                    continue
                if on_gpu:
                    stage = stage.to(dev, non_blocking=True)
                valid = torch.arange(S, device=stage.device)[None, :] < stage[:, S:]
                tile = torch.where(valid, stage[:, :S], 0)       # whatever sits past a row's length is not a token
                parts.append(self.encoder.forward(tile, valid.int(), pooling=self.pooling, normalise=self.normalize))
            res = self._stage_out[: n * self.dimensions].view(n, self.dimensions)
            res.copy_(dev_out if lens_path else torch.cat(parts), non_blocking=False)      # one device-to-host copy, into pinned memory
            out[order] = res.numpy()
        return out
