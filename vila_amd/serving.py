"""Serving shim: `generate_content` + an OpenAI-style `/chat/completions` endpoint over the HIP model.

Mirrors the parts of the reference a client sees:
  * `LlavaLlamaModel.generate_content(prompt)` (llava/model/llava_arch.py:836-948): a prompt is a string or a list of parts (strings and
    images); media are extracted in order, pre-processed, the text gets one `<image>` token per image, greedy generation, decoded text
  * `server.py:171-290`: POST /chat/completions with OpenAI-style messages (`text` / `image_url` / `video_url` parts, base64 data URLs), the
    response object layout, `stream=True` as server-sent `chat.completion.chunk` events that leave WHILE the reply is generated
    (`TextStream` = `transformers.TextIteratorStreamer`'s release rule, fed by `llm.generate(streamer=...)` or by the continuous batcher)
  * `process_image` / `process_images` (llava/mm_utils.py:442-541): every `image_aspect_ratio` mode — resize, pad, dynamic (the NVILA-Lite
    tiler), dynamic_s2 (the NVILA tiler)
What stays in the reference: conversation templates beyond the Qwen2 chat form, video FILE decoding (OpenCV).  Structured output (the reference's
`response_format`, compiled there with xgrammar) is served by `generate_content(response_format= / guided_choice= / guided_regex=)` and the endpoint's request fields of the same names through a token
automaton on the device (`vila_amd/constrain.py`); free-form `json_object` is not.
The tokenizer is whatever the checkpoint ships (`transformers.AutoTokenizer`), handed in by the caller; images are pre-processed the way
`SiglipImageProcessor` does for NVILA (resize to the tower's resolution, bicubic, rescale 1/255, normalise mean = std = 0.5).
"""
from __future__ import annotations

import base64
import glob
import io
import itertools
import json
import os
import re
import threading
import time
import uuid
from collections import OrderedDict
from types import SimpleNamespace
from typing import Any, Dict, Iterator, List, Optional, Sequence, Union

import numpy as np
import torch

from .modules import _eos_set

IMAGE_TOKEN = "<image>"
MEDIA_TOKENS = {"image": "<image>", "video": "<vila/video>"}          # llava/constants.py:32-35
_DATA_URL = re.compile(r"^data:image/(png|jpe?g);base64,(.*)$", re.S)


def _to_pil(img):
    """PIL image / HxWx3 uint8 array / 3xHxW (or HxWx3) tensor in [0,1] or [0,255] -> PIL RGB image."""
    from PIL import Image
    if hasattr(img, "convert"):
        return img.convert("RGB")                                    # mm_utils.py:452
    if isinstance(img, torch.Tensor):
        x = img.detach().float().cpu()
        if x.dim() == 3 and x.shape[0] == 3 and x.shape[-1] != 3:
            x = x.permute(1, 2, 0)
        if x.max() <= 1.5:
            x = x * 255.0
        img = x.round().clamp(0, 255).to(torch.uint8).numpy()
    return Image.fromarray(np.ascontiguousarray(np.asarray(img, dtype=np.uint8)), "RGB")


def preprocess_image(img, size: int) -> torch.Tensor:
    """-> [3, size, size] float32 in [-1, 1], the pixels `SiglipImageProcessor.preprocess` hands the tower (mm_utils.py:442-541, row a1): PIL
    bicubic resize to size x size (skipped when the image already has that size), rescale by 1/255, normalise with mean = std = 0.5.
    PIL does the resampling — the reference's input producer is kept as it is, so the pixels ARE the reference's
    (tests/test_s2_tiler_cpu.py holds this function to HF-processor-executed vectors)."""
    from PIL import Image
    pil = _to_pil(img)
    if pil.size != (size, size):
        pil = pil.resize((size, size), resample=Image.BICUBIC)
    x = torch.from_numpy(np.asarray(pil, dtype=np.uint8).copy()).permute(2, 0, 1).float()
    return (x * (1.0 / 255.0) - 0.5) / 0.5


def process_image(img, cfg, enable_dynamic_res: bool = False, enable_dynamic_s2: bool = False, max_tiles: Optional[int] = None):
    """`process_image` (mm_utils.py:442-523) for the SigLIP tower, `cfg.aspect_mode` standing for `data_args.image_aspect_ratio`:
      * "dynamic_s2" + enable_dynamic_s2 -> ([n_tiles, 3, S, S], block_size): the tiles of every scale (`dynamic_s2_preprocess`)
      * "dynamic*"   + enable_dynamic_res -> [n_tiles, 3, S, S]: the grid closest to the picture's aspect ratio + a thumbnail
        (`dynamic_preprocess`, min_tiles .. max_tiles, `max_tiles=` overrides the config's)
      * "resize" -> PIL resize to S x S; "pad" -> centred on a square of the processor's mean colour (`expand2square`), then the processor
      * anything else -> the processor's default, which for SigLIP is the resize
    every tile / picture through `preprocess_image` (= `SiglipImageProcessor.preprocess`).  Pinned by tests/golden/dynamic_tiles.npz = the
    reference's own function executed on the same pictures."""
    from .host import dynamic_preprocess, dynamic_s2_preprocess, expand2square
    pil = _to_pil(img)
    size = cfg.vision.image_size
    mode = cfg.aspect_mode
    if "dynamic_s2" in mode and enable_dynamic_s2:
        tiles, block_size = dynamic_s2_preprocess(pil, list(cfg.s2_scales), int(cfg.max_tiles), size)
        return torch.stack([preprocess_image(t, size) for t in tiles]), block_size
    if "dynamic" in mode and enable_dynamic_res:
        max_num = int(max_tiles) if max_tiles is not None else int(cfg.max_tiles)
        tiles = dynamic_preprocess(pil, min_num=int(cfg.min_tiles), max_num=max_num, image_size=size)
        return torch.stack([preprocess_image(t, size) for t in tiles])
    if mode == "resize":
        pil = pil.resize((size, size))
    if mode == "pad":
        pil = expand2square(pil, tuple(int(x * 255) for x in (0.5, 0.5, 0.5)))           # SiglipImageProcessor.image_mean
    return preprocess_image(pil, size)


def process_images(images, cfg, enable_dynamic_res: bool = False, max_tiles: Optional[int] = None) -> torch.Tensor:
    """`process_images` (mm_utils.py:526-541): every picture through `process_image`; tiled pictures ([n, 3, S, S] each) are concatenated,
    whole ones stacked; pictures whose results differ in shape (different tile counts) are refused with the reference's message."""
    new_images = [process_image(im, cfg, enable_dynamic_res=enable_dynamic_res, max_tiles=max_tiles) for im in images]
    if not all(x.shape == new_images[0].shape for x in new_images):
        raise ValueError("The shape of images in new_images is different!")
    return torch.cat(new_images, dim=0) if new_images[0].dim() == 4 else torch.stack(new_images, dim=0)


def preprocess_media(images, cfg):
    """The media half of `generate_content` (llava_arch.py:857-879): ONE image under a tiling recipe becomes its tiles — `dynamic_s2`: the
    tiles of every scale with media_config["image"]["block_sizes"] = [block_size]; `dynamic`: the aspect-ratio grid + thumbnail (the prompt
    then carries one `<image>\n` per tile, see `prepare_prompt`); otherwise every image goes through `process_images` whole.
    -> (list of [3, size, size] float tensors, media_config)."""
    mode = cfg.aspect_mode
    if len(images) == 1 and mode == "dynamic_s2":
        tiles, block_size = process_image(images[0], cfg, enable_dynamic_s2=True)
        return list(tiles), {"image": {"block_sizes": [block_size]}}
    if len(images) == 1 and mode == "dynamic":
        return list(process_image(images[0], cfg, enable_dynamic_res=True)), {}
    return ([] if not images else list(process_images(images, cfg))), {}


def load_image(url: str):
    """`data:image/...;base64,` URLs (server.py:56-75).  Remote http(s) fetches are left to the caller (no network in this build)."""
    m = _DATA_URL.match(url)
    if not m:
        raise ValueError("only base64 data URLs (data:image/png|jpeg;base64,...) are supported by this shim")
    from PIL import Image
    return Image.open(io.BytesIO(base64.b64decode(m.group(2)))).convert("RGB")


class Video:
    """A video prompt part: its already-extracted frames (images, or one [T, H, W, 3] array).  In this snapshot of the reference a `Video` part
    becomes `num_video_frames` `<image>` tokens and its frames join the IMAGE list (llava/utils/media.py:114-119); picking the frames out of a
    file (`_load_video`, cv2) stays with the caller."""

    def __init__(self, frames) -> None:
        self.frames = list(frames)


_VIDEO_URL = re.compile(r"^data:video/(mp4);base64,(.*)$")            # server.py:57


def video_frame_indices(frame_count: int, num_frames: int, fps: float = 0.0, video_fps: float = 0.0) -> List[int]:
    """Which frames of a `frame_count`-frame video the reference keeps (llava/utils/media.py:62-72): with `fps > 0` one frame every 1 / fps
    seconds of the video's duration, clamped to `num_frames`; else `num_frames` positions spread evenly over the whole video
    (`np.round(np.linspace(0, n - 1, num_frames))`).  Pinned by tests/golden/video_sampling_ref.json = the reference's own `_load_video`
    executed over a synthetic capture."""
    if fps and fps > 0:
        duration = frame_count / video_fps if video_fps > 0 else 0    # (a container without a frame rate selects nothing: the loader raises)
        stamps = np.arange(0, duration, 1.0 / fps)[:num_frames]
        return [int(t * video_fps) for t in stamps]
    return [int(i) for i in np.round(np.linspace(0, frame_count - 1, num_frames)).astype(int)]


def load_video_frames(path: str, num_frames: int = 8, fps: float = 0.0):
    """`_load_video` (llava/utils/media.py:39-86): a DIRECTORY of frame images (sorted, `num_frames` spread evenly) or a video file (needs
    OpenCV, which this image does not ship: imported lazily, a missing module is reported as such) -> list of PIL images."""
    from PIL import Image
    if os.path.isdir(path):
        files = sorted(glob.glob(os.path.join(path, "*")))
        if not files:
            raise ValueError(f"Video '{path}' has no frames.")
        return [Image.open(files[i]).convert("RGB") for i in video_frame_indices(len(files), num_frames)]
    try:
        import cv2
    except ImportError as e:
        raise RuntimeError("decoding a video FILE needs OpenCV (cv2), as in the reference (llava/utils/media.py:47); pass a directory of frames "
                           "or a serving.Video(frames) part instead") from e
    cap = cv2.VideoCapture(path)
    video_fps = cap.get(cv2.CAP_PROP_FPS)
    n = int(cap.get(cv2.CAP_PROP_FRAME_COUNT))
    while n > 0:                                                     # the container's frame count may overshoot (:53-59)
        cap.set(cv2.CAP_PROP_POS_FRAMES, n - 1)
        if cap.grab():
            break
        n -= 1
    else:
        raise ValueError(f"Video '{path}' has no frames.")
    frames = {}
    idx = video_frame_indices(n, num_frames, fps, video_fps)
    for i in idx:
        if i in frames:
            continue
        cap.set(cv2.CAP_PROP_POS_FRAMES, i)
        ok, frame = cap.read()
        if ok:
            frames[i] = Image.fromarray(cv2.cvtColor(frame, cv2.COLOR_BGR2RGB))
    return [frames[i] for i in idx if i in frames]


def load_video_url_frames(url: str, num_frames: int = 8, fps: float = 0.0):
    """A request's `video_url` -> frames.  The reference writes the body to a temp file that stays (server.py:60-78); here the file lives
    only while it is decoded, so a long-running server does not keep one video per request on disk."""
    import shutil
    path = load_video(url)
    try:
        frames = load_video_frames(path, num_frames=num_frames, fps=fps)
        if not frames:                       # `_load_video` itself returns [] here (media.py:62-86, pinned); a REQUEST with no frames is refused
            raise ValueError("video_url: no frame could be selected (a container that reports no frame rate under the fps rule, or "
                             "unreadable frames)")
        return frames
    finally:
        shutil.rmtree(os.path.dirname(path), ignore_errors=True)


def load_video(url: str) -> str:
    """`load_video` of server.py:60-78: a `data:video/mp4;base64,` URL is written to a temporary .mp4 whose path is returned.  Remote http(s)
    fetches are left to the caller (no network in this build); local paths are NOT accepted from a request (the Python API takes them:
    `load_video_frames(path)` / `Video(frames)`)."""
    m = _VIDEO_URL.match(url)
    if m:
        import tempfile
        path = os.path.join(tempfile.mkdtemp(), f"{uuid.uuid5(uuid.NAMESPACE_DNS, url)}.mp4")
        with open(path, "wb") as f:
            f.write(base64.b64decode(m.group(2)))
        return path
    raise ValueError(f"Invalid video url: {url[:64]}")


def _split_prompt(prompt: Union[str, Sequence[Any]]):
    """llava/utils/media.py:93-122 (extract_media): text with exactly one `<image>` per image part (the "\n" after an image is NOT
    text: BasicImageEncoder appends it as an embedding, encoders/image/basic.py:22-27), images in order; a `Video` part is one `<image>`
    per frame (:114-119); media tokens typed by the user inside a text part are removed and the part stripped (:104-108).
    Pinned by tests/golden/prompt_split_ref.json = the reference's own function executed on the same prompts."""
    text, images = "", []
    for part in ([prompt] if isinstance(prompt, str) else prompt):
        if isinstance(part, str):
            for token in MEDIA_TOKENS.values():                       # every media token, the video one included (media.py:103-106)
                if token in part:
                    part = part.replace(token, "").strip()
            text += part
        elif isinstance(part, Video):
            images.extend(part.frames)
            text += IMAGE_TOKEN * len(part.frames)
        else:
            images.append(part)
            text += IMAGE_TOKEN
    return text, images


def prepare_prompt(prompt: Union[str, Sequence[Any]], cfg):
    """Prompt parts -> (text, tiles, media_config): `extract_media` + the media branch of `generate_content` (llava_arch.py:842-879).  Under
    the `dynamic` recipe a single image's `<image>` becomes one `<image>\n` per tile (:864-866; the dataset path builds the same text,
    mm_utils.py:408-424).  The text is stripped like `tokenize_conversation` does with every message (llava/utils/tokenizer.py:77-78)."""
    text, images = _split_prompt(prompt)
    tiles, media_config = preprocess_media(images, cfg)
    if len(images) == 1 and cfg.aspect_mode == "dynamic":
        text = text.replace(IMAGE_TOKEN, f"{IMAGE_TOKEN}\n" * len(tiles))
    return text.strip(), tiles, media_config


def chat_text(text: str, system: Optional[str] = None) -> str:
    """Qwen2 chat form with the generation prompt appended (tokenize_conversation(add_generation_prompt=True), llava/utils/tokenizer.py)."""
    s = f"<|im_start|>system\n{system}<|im_end|>\n" if system else ""
    return s + f"<|im_start|>user\n{text}<|im_end|>\n<|im_start|>assistant\n"


def prompt_text(tokenizer, text: str, system: Optional[str] = None) -> str:
    """The string the model is prompted with: the tokenizer's OWN chat template with the generation prompt appended, exactly what
    `generate_content` builds (`tokenize_conversation(conversation, tokenizer, add_generation_prompt=True)`, llava_arch.py:921 ->
    llava/utils/tokenizer.py:109-113) — Qwen2's template, for one, supplies a default system turn.  A tokenizer without a template (the
    synthetic stand-ins) gets the bare Qwen2 chat form (`chat_text`)."""
    if getattr(tokenizer, "chat_template", None) and hasattr(tokenizer, "apply_chat_template"):
        turns = ([{"role": "system", "content": system}] if system else []) + [{"role": "user", "content": text}]
        return tokenizer.apply_chat_template(turns, add_generation_prompt=True, tokenize=False)
    return chat_text(text, system)


def encode_with_images(tokenizer, text: str, image_token_id: int) -> torch.Tensor:
    """tokenizer_image_token (llava/mm_utils.py): tokenize the pieces between <image> tags, put the media id in between."""
    ids: List[int] = []
    for i, piece in enumerate(text.split(IMAGE_TOKEN)):
        if i:
            ids.append(image_token_id)
        if piece:
            ids.extend(tokenizer(piece, add_special_tokens=False).input_ids if callable(tokenizer) else tokenizer.encode(piece))
    return torch.tensor(ids, dtype=torch.int64)


def _is_cjk(cp: int) -> bool:
    """transformers/generation/streamers.py `TextStreamer._is_chinese_char`: the CJK Unified Ideographs blocks."""
    return (0x4E00 <= cp <= 0x9FFF or 0x3400 <= cp <= 0x4DBF or 0x20000 <= cp <= 0x2A6DF or 0x2A700 <= cp <= 0x2B73F or 0x2B740 <= cp <= 0x2B81F
            or 0x2B820 <= cp <= 0x2CEAF or 0xF900 <= cp <= 0xFAFF or 0x2F800 <= cp <= 0x2FA1F)


class TextStream:
    """Token ids in, text pieces out, across threads — what `transformers.TextIteratorStreamer` is to the reference's server
    (server.py:22, 241-270: `for new_text in streamer`).  `put` / `end` follow `TextStreamer.put` / `end` token by token: the cache of
    undecoded tokens is decoded whole; text up to the last space is released (a word may still change with the next token), everything
    after a newline (the cache restarts) or a CJK character.  Pieces — empty ones too, as HF queues them — wait in a queue for the
    consumer; `fail(exc)` makes the consumer raise.  Pinned by tests/test_serving_cpu.py against HF's class run on the same token sequences."""

    _END = object()

    def __init__(self, tokenizer, skip_special_tokens: bool = True, timeout: Optional[float] = None):
        import queue
        self.tokenizer, self.skip_special_tokens, self.timeout = tokenizer, skip_special_tokens, timeout
        self._cache: List[int] = []
        self._print_len = 0
        self._q: "queue.Queue" = queue.Queue()
        self._ended = False
        self.token_ids: List[int] = []                   # everything that was put (observability / tests)

    def _decode(self) -> str:
        return self.tokenizer.decode(self._cache, skip_special_tokens=self.skip_special_tokens)

    def put(self, value) -> None:
        ids = value.tolist() if hasattr(value, "tolist") else value
        if isinstance(ids, int):
            ids = [ids]
        if ids and isinstance(ids[0], (list, tuple)):
            if len(ids) > 1:
                raise ValueError("TextStreamer only supports batch size 1")
            ids = ids[0]
        for t in ids:
            self.token_ids.append(int(t))
            self._cache.append(int(t))
            text = self._decode()
            if text.endswith("\n"):
                piece = text[self._print_len:]
                self._cache, self._print_len = [], 0
            elif len(text) > 0 and _is_cjk(ord(text[-1])):
                piece = text[self._print_len:]
                self._print_len += len(piece)
            else:
                piece = text[self._print_len: text.rfind(" ") + 1]
                self._print_len += len(piece)
            self._q.put(piece)

    def end(self) -> None:
        piece = ""
        if self._cache:
            piece = self._decode()[self._print_len:]
            self._cache, self._print_len = [], 0
        self._q.put(piece)
        self._q.put(self._END)
        self._ended = True

    def finish(self, text: str) -> None:
        """For a producer whose `generate` took no streamer (it never called `put` / `end`): the whole reply as one piece, then the end."""
        if not self._ended:
            if not self.token_ids:
                self._q.put(text)
            self.end()

    def fail(self, exc: BaseException) -> None:
        self._q.put(exc)
        self._ended = True

    def __iter__(self):
        return self

    def __next__(self) -> str:
        item = self._q.get(timeout=self.timeout)
        if item is self._END:
            raise StopIteration
        if isinstance(item, BaseException):
            raise item
        return item


def sse_chunks(pieces, model_name: str, stop_str: str = "<|im_end|>") -> Iterator[str]:
    """The `chunk_generator` of server.py:243-268: text pieces -> server-sent `chat.completion.chunk` events.  A lone " " is held back and
    prepended to the next piece; a piece that ends with the stop string loses it (and is stripped); empty pieces send nothing; `[DONE]` closes."""
    prepend_space = False
    chunk_id = 0
    for new_text in pieces:
        if new_text == " ":
            prepend_space = True
            continue
        if stop_str and new_text.endswith(stop_str):
            new_text = new_text[: -len(stop_str)].strip()
            prepend_space = False
        elif prepend_space:
            new_text = " " + new_text
            prepend_space = False
        if len(new_text):
            chunk = {"id": str(chunk_id), "object": "chat.completion.chunk", "created": time.time(), "model": model_name,
                     "choices": [{"delta": {"content": new_text}}]}
            yield f"data: {json.dumps(chunk)}\n\n"
    yield "data: [DONE]\n\n"


def _eos_of(tokenizer, eos_token_id=None):
    """The ids generation stops on: the caller's, else the tokenizer's `stop_token_ids` (what `default_generation_config` hands HF as
    `eos_token_id`, llava_arch.py:961-962: the end-of-turn tokens `infer_stop_tokens` read off the chat template), else its EOS."""
    if eos_token_id is not None:
        return eos_token_id
    stop = getattr(tokenizer, "stop_token_ids", None)
    if stop:
        return list(stop) if len(stop) > 1 else stop[0]
    return getattr(tokenizer, "eos_token_id", None)


PENALTY_NEUTRAL = dict(repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0)


def _penalties_of(gen) -> Dict[str, float]:
    """The non-neutral penalties among a request's keywords, as keywords of `llm.generate`: {} for a request that asks for none (None or the neutral
    1 / 0 / 0), which is then served exactly as a request without the fields."""
    return {k: float(gen[k]) for k, v in PENALTY_NEUTRAL.items() if gen.get(k) is not None and float(gen[k]) != v}


LOGPROBS_MAX_TOP = 20


class ReplyWithLogprobs(str):
    """A reply that carries its per-token log-probabilities: the text, as every caller that treats the result as text expects it, with `.logprobs`,
    the entries in OpenAI layout (`logprob_entries`)."""

    def __new__(cls, text: str, logprobs: List[Dict[str, Any]]):
        self = super().__new__(cls, text)
        self.logprobs = logprobs
        return self


def _logprobs_of(logprobs, top_logprobs) -> Optional[int]:
    """A request's `logprobs` / `top_logprobs` -> None for a request that asks for none (served exactly as a request without the fields), else the
    number of alternatives per token (0..20, OpenAI's limit).  top_logprobs without logprobs is an error, as it is there."""
    if not logprobs:
        if top_logprobs is not None:
            raise ValueError("`top_logprobs` needs `logprobs`: true")
        return None
    k = 0 if top_logprobs is None else top_logprobs
    if isinstance(k, bool) or not isinstance(k, int) or not 0 <= k <= LOGPROBS_MAX_TOP:
        raise ValueError(f"`top_logprobs` has to be an integer in 0..{LOGPROBS_MAX_TOP}, but is {top_logprobs!r}")
    return k


def logprob_entries(tokenizer, toks: Sequence[int], token_logprobs, top_logprobs, top_ids, k: int) -> List[Dict[str, Any]]:
    """The `logprobs.content` list of an OpenAI chat completion for the reply tokens `toks`: per token {"token", "logprob", "bytes",
    "top_logprobs": [{"token", "logprob", "bytes"}, ... k of them]}, token = tokenizer.decode([id]), bytes = its UTF-8 bytes.  The three records
    hold at least len(toks) positions (lists or tensors: [n], [n, >= k], [n, >= k]); what lies behind is ignored, so the entries are cut exactly
    where the caller cut the tokens."""
    as_list = lambda v: v.tolist() if hasattr(v, "tolist") else list(v)
    tl, pl, pi = as_list(token_logprobs), as_list(top_logprobs), as_list(top_ids)

    def one(t, lp):
        piece = tokenizer.decode([int(t)])
        return {"token": piece, "logprob": float(lp), "bytes": list(piece.encode("utf-8"))}
    out = []
    for j, t in enumerate(toks):
        entry = one(t, tl[j])
        entry["top_logprobs"] = [one(i, l) for i, l in zip(pi[j][:k], pl[j][:k]) if int(i) >= 0] if k else []
        out.append(entry)
    return out


_COMPILERS: "OrderedDict[Any, Any]" = OrderedDict()
_COMPILERS_KEPT = 4              # tokenizers whose compiler (a byte table of the vocabulary and an LRU of automata) is kept; the oldest goes
STRUCTURED_FIELDS = ("response_format", "guided_choice", "guided_regex")


def constraint_compiler(tokenizer, vocab_size: int, eos_token_id=None, max_table: Optional[int] = None, max_classes: Optional[int] = None):
    """The `ConstraintCompiler` of a tokenizer (byte-level BPE: `token_bytes_from_tokenizer`), kept per (tokenizer, vocabulary, EOS set, caps) with
    its LRU of compiled automata, as xgrammar's GrammarCompiler keeps its cache.  At most `_COMPILERS_KEPT` are kept, least recently used first out.
    max_table / max_classes: the caps of the session that will hold the automata (default: `generate`'s)."""
    from .constrain import MAX_CLASSES, ConstraintCompiler, token_bytes_from_tokenizer
    eos = tuple(sorted(int(e) for e in _eos_set(_eos_of(tokenizer, eos_token_id)) if 0 <= int(e) < int(vocab_size)))
    key = (id(tokenizer), int(vocab_size), eos, max_table, max_classes)
    got = _COMPILERS.get(key)
    if got is None or got[0] is not tokenizer:           # (the tokenizer is held with its entry, so its id cannot be another object's)
        got = (tokenizer, ConstraintCompiler(token_bytes_from_tokenizer(tokenizer, vocab_size), eos, max_table=max_table,
                                             max_classes=MAX_CLASSES if max_classes is None else int(max_classes)))
    _COMPILERS[key] = got
    _COMPILERS.move_to_end(key)
    while len(_COMPILERS) > _COMPILERS_KEPT:
        _COMPILERS.popitem(last=False)
    return got[1]


def structured_of(gen) -> Dict[str, Any]:
    """The structured-output fields a request carries, as keywords of `generate_content`: {} for a request that asks for none (absent, None, or a
    `response_format` of type "text"), which is then served exactly as a request without the fields.  More than one is an error."""
    from .constrain import response_format_spec
    asks = {k: gen[k] for k in STRUCTURED_FIELDS if gen.get(k) is not None}
    if "response_format" in asks and response_format_spec(asks["response_format"]) is None:
        del asks["response_format"]
    if len(asks) > 1:
        raise ValueError(f"structured output: give one of response_format / guided_choice / guided_regex (got {sorted(asks)})")
    return asks


def check_structured_request(gen, stream: bool) -> Dict[str, Any]:
    """`structured_of(gen)`, refused together with `stream`: a constrained reply is not streamed."""
    asks = structured_of(gen)
    if asks and stream:
        raise ValueError("structured output (response_format / guided_choice / guided_regex) is not served together with `stream`: true")
    return asks


def constraint_of(gen, compiler):
    """The automaton a request asks for, or None: `response_format` (the reference's ResponseFormat shape: `type` plus `json_schema.schema`; laid
    out with indent=2, as the reference asks xgrammar), `guided_choice` (a list of strings) or `guided_regex` (a pattern) — one of them.  A
    compile error (an unsupported schema, `json_object`, a constraint the vocabulary cannot spell) is a ValueError."""
    from .constrain import response_format_spec
    spec = response_format_spec(gen.get("response_format"))
    asked = [k for k, v in (("response_format", spec), ("guided_choice", gen.get("guided_choice")), ("guided_regex", gen.get("guided_regex"))) if v is not None]
    if len(asked) > 1:
        raise ValueError(f"structured output: give one of response_format / guided_choice / guided_regex (got {asked})")
    if not asked:
        return None
    if spec is not None:
        return compiler.json_schema(spec[1], indent=2)
    if gen.get("guided_choice") is not None:
        return compiler.choice(list(gen["guided_choice"]))
    return compiler.regex(gen["guided_regex"])


def generate_content(model, tokenizer, prompt: Union[str, Sequence[Any]], max_new_tokens: int = 128, system: Optional[str] = None,
                     eos_token_id=None, device: Optional[str] = None, temperature: float = 0.0, top_p: float = 1.0, top_k: int = 50,
                     seed: Optional[int] = None, streamer=None, prompt_lookup_num_tokens: Optional[int] = None, spec_sample: bool = False,
                     repetition_penalty: Optional[float] = None, presence_penalty: Optional[float] = None,
                     frequency_penalty: Optional[float] = None, logprobs: Optional[bool] = None, top_logprobs: Optional[int] = None,
                     response_format=None, guided_choice: Optional[Sequence[str]] = None, guided_regex: Optional[str] = None,
                     any_top_k: bool = False, spec_processed: bool = False) -> str:
    """Text + images in, decoded reply out — the contract of `LlavaLlamaModel.generate_content` for image / text prompts.
    temperature > 0 samples (server.py:185-187: do_sample = temperature > 0, with the request's top_p and HF's default top_k = 50).
    prompt_lookup_num_tokens=k: speculative decoding with k lookup drafts per step (`llm.generate(prompt_lookup_num_tokens=)`); the reply is
    the greedy reply.  A sampled request ignores it unless spec_sample=True (default False), which passes both on
    (`llm.generate(do_sample=True, prompt_lookup_num_tokens=k, spec_sample=True)`, top_k in 1..64): the reply is then the one the same sampled
    request gives without drafts, a draft being accepted exactly when the request's own draw hits it.  any_top_k=True (default False) passes
    `any_top_k=True` on with them, and the speculating request may carry any top_k >= 0 (0 = no top-k filter).
    streamer: a `TextStream` (or any HF streamer) that receives the new tokens while they are generated (`llm.generate(streamer=...)`).
    repetition_penalty / presence_penalty / frequency_penalty: passed on to `llm.generate` when they are not neutral (1 / 0 / 0 or None); a
    penalised request is not speculated (prompt_lookup_num_tokens is dropped for it) unless spec_processed=True, below.
    logprobs=True (with top_logprobs = 0..20 alternatives per token): the reply comes back as a `ReplyWithLogprobs` — the same text, with
    `.logprobs`, one OpenAI-layout entry per reply token (`logprob_entries`), cut exactly where the text's tokens are cut: the EOS and what follows
    are dropped.  The numbers are RAW: the model's own distribution, independent of temperature, top_p and penalties (`llm.generate(logprobs=)`).
    Such a request is not speculated either, unless spec_processed=True.
    response_format (the reference's `ResponseFormat`: {"type": "json_schema", "json_schema": {"schema": ...}}, an object or a dict), guided_choice
    (a list of strings) or guided_regex (a pattern): structured output — the reply is held to the schema (in the layout of
    `json.dumps(obj, indent=2)`), to one of the strings, or to the pattern, by a token automaton on the device (`llm.generate(constraint=)`,
    `vila_amd/constrain.py` has the served subsets; `{"type": "json_object"}` is not served).  max_new_tokens can still cut the reply before it is
    complete.  Such a request is not streamed, and not speculated unless spec_processed=True.
    spec_processed=True (default False): a penalised, logprob or structured request KEEPS prompt_lookup_num_tokens instead of dropping it, and
    `spec_processed=True` travels to `llm.generate` with it (the processed verify step); the reply is the one the same request gives without drafts."""
    asks = check_structured_request(dict(response_format=response_format, guided_choice=guided_choice, guided_regex=guided_regex), streamer is not None)
    constraint = None
    if asks:
        from .modules import HipQwen2ForCausalLM as _Llm
        constraint = constraint_of(asks, constraint_compiler(tokenizer, model.cfg.llm.vocab_size, eos_token_id,
                                                             max_table=_Llm.CONSTRAIN_MAX_STATES * _Llm.CONSTRAIN_MAX_CLASSES))
        if not spec_processed:
            prompt_lookup_num_tokens = None
    pen = _penalties_of(dict(repetition_penalty=repetition_penalty, presence_penalty=presence_penalty, frequency_penalty=frequency_penalty))
    n_top = _logprobs_of(logprobs, top_logprobs)
    if (pen or n_top is not None) and not spec_processed:
        prompt_lookup_num_tokens = None
    cfg = model.cfg
    dev = device or str(model.device)
    text, tiles, media_config = prepare_prompt(prompt, cfg)
    ids = encode_with_images(tokenizer, prompt_text(tokenizer, text, system), cfg.image_token_id)[None].to(dev)
    media = {"image": [t.to(device=dev, dtype=torch.bfloat16) for t in tiles]}
    eos = _eos_of(tokenizer, eos_token_id)
    gen = dict(max_new_tokens=max_new_tokens, eos_token_id=eos)
    if temperature and temperature > 0:
        gen.update(do_sample=True, temperature=float(temperature), top_p=float(top_p), top_k=int(top_k), seed=seed)
        if spec_sample and prompt_lookup_num_tokens is not None:
            gen.update(prompt_lookup_num_tokens=int(prompt_lookup_num_tokens), spec_sample=True)
            if any_top_k:                              # (keyword only when asked: a call without it makes the call it always made)
                gen.update(any_top_k=True)
    elif prompt_lookup_num_tokens is not None:
        gen.update(prompt_lookup_num_tokens=int(prompt_lookup_num_tokens))
    if spec_processed and "prompt_lookup_num_tokens" in gen and (pen or n_top is not None or constraint is not None):
        gen.update(spec_processed=True)                # (keyword only for a request that needs it: every other call is the one it always was)
    if streamer is not None:
        gen.update(streamer=streamer)
    gen.update(pen)
    if constraint is not None:                         # (keyword only when asked, likewise)
        gen.update(constraint=constraint)
    lp = None
    if n_top is not None:                              # (keyword only when asked: a request without the fields makes the call it always made)
        out, lp = model.generate(input_ids=ids, media=media, media_config=media_config, logprobs=n_top, **gen)
    else:
        out = model.generate(input_ids=ids, media=media, media_config=media_config, **gen)
    toks = out[0].tolist()
    stop = _eos_set(eos)
    for k, t in enumerate(toks):                       # HF returns the EOS as the last token; decode(skip_special_tokens) drops it
        if t in stop:
            toks = toks[:k]
            break
    text = tokenizer.decode(toks, skip_special_tokens=True).strip()
    if lp is not None:
        return ReplyWithLogprobs(text, logprob_entries(tokenizer, toks, lp.token_logprobs[0], lp.top_logprobs[0], lp.top_ids[0], n_top))
    return text


class ChatOverflow(ValueError):
    """A turn that does not fit the session's KV cache.  The session is unchanged and stays usable (ask something shorter, or `reset()`)."""


class ChatSession:
    """A conversation that keeps its KV cache: every `ask` prefills only the NEW tokens onto the cache (`llm.generate(cache=, past_len=)`), so a
    follow-up question re-encodes no earlier image and re-prefills no earlier turn.

    The session owns one cache of `max_ctx` positions and three pieces of state:
      ids       the conversation's token ids so far, media as their placeholder ids (what a one-shot `generate` of the whole conversation is fed);
      cached    the number of leading POSITIONS of the cache whose K/V are valid (an image placeholder is many positions);
      the last emitted token, which has NOT been fed yet: after `generate` returns n tokens on top of P cached positions and S new ones the cache
      holds P + S + n - 1 — rows beyond that may hold steps the device ran past the EOS, or rejected drafts, and count for nothing.
    So the next turn's new tokens open with that last token, then the end-of-turn marker if the reply was cut by max_new_tokens rather than by it,
    the separator and the new user turn in the Qwen2 chat form (`chat_text`, the template every NVILA recipe runs).  Media of a later turn are
    encoded and spliced for the new part only.  gen_defaults / `ask(**gen)`: keyword arguments of `llm.generate` (do_sample, temperature, top_k,
    top_p, seed, prompt_lookup_num_tokens, spec_sample, spec_processed, streamer, repetition_penalty, presence_penalty, frequency_penalty, ...).  The penalties
    count what the CURRENT turn has generated: every `ask` is a request of its own, earlier turns are prompt."""

    TURN_END = "<|im_end|>"

    def __init__(self, model, tokenizer, max_ctx: int = 4096, system: Optional[str] = None, eos_token_id=None, **gen_defaults):
        self.model, self.tokenizer, self.max_ctx, self.system = model, tokenizer, int(max_ctx), system
        self.eos = _eos_of(tokenizer, eos_token_id)
        self.gen_defaults = dict(gen_defaults)
        self.cache = None
        self.reset()

    def reset(self) -> None:
        """Back to an empty conversation (the cache's memory is kept and overwritten)."""
        self.ids: List[int] = []
        self.cached = 0
        self._last: Optional[int] = None          # the last emitted token (in `ids`, not in the cache)
        self._closed = True                       # the last reply ended with a stop token of its own

    def _new_ids(self, text: str) -> List[int]:
        """The ids this turn adds in front of the reply: the first turn's prompt, or end-of-turn (if missing) + separator + the user turn."""
        image_id = self.model.cfg.image_token_id
        if self._last is None:
            return encode_with_images(self.tokenizer, prompt_text(self.tokenizer, text, self.system), image_id).tolist()
        return encode_with_images(self.tokenizer, ("" if self._closed else self.TURN_END) + "\n" + chat_text(text), image_id).tolist()

    def ask(self, prompt: Union[str, Sequence[Any]], max_new_tokens: int = 128, **gen) -> str:
        if max_new_tokens < 1:
            raise ValueError(f"max_new_tokens has to be a positive integer, but is {max_new_tokens}")
        model, dev = self.model, str(self.model.device)
        text, tiles, media_config = prepare_prompt(prompt, model.cfg)
        new = self._new_ids(text)
        fed = ([] if self._last is None else [self._last]) + new              # what is prefilled: the token never fed comes first
        media = {"image": [t.to(device=dev, dtype=torch.bfloat16) for t in tiles]}
        with torch.inference_mode():
            embeds, _, _ = model._embed(torch.tensor([fed], dtype=torch.int64, device=dev), media, media_config, None, None)
        P, S = self.cached, int(embeds.shape[1])
        if P + S + max_new_tokens > self.max_ctx:
            raise ChatOverflow(f"the turn does not fit the session's cache: {P} cached + {S} new + {max_new_tokens} to generate > max_ctx {self.max_ctx} "
                               "(the session is unchanged; reset() starts a new conversation)")
        if self.cache is None:
            self.cache = model.llm.new_cache(self.max_ctx)
        kw = {**self.gen_defaults, **gen}
        kw.setdefault("eos_token_id", self.eos)
        if kw.get("prompt_lookup_num_tokens") is not None and kw.get("prompt_ids") is None:
            kw["prompt_ids"] = torch.tensor(self.ids + new, dtype=torch.int64, device=dev)
        if P:
            kw["past_len"] = P
        out = model.llm.generate(inputs_embeds=embeds, max_new_tokens=max_new_tokens, cache=self.cache, **kw)
        toks = [int(t) for t in out[0].tolist()]
        stop = _eos_set(kw["eos_token_id"], model.cfg.llm.eos_token_id)
        # the state moves only now: a turn that raised left it as it was
        self.ids.extend(new)
        self.ids.extend(toks)
        self.cached = P + S + len(toks) - 1
        self._last = toks[-1]
        self._closed = toks[-1] in stop
        reply = toks[:-1] if self._closed else toks
        return self.tokenizer.decode(reply, skip_special_tokens=True).strip()


def generate_content_batch(model, tokenizer, prompts: Sequence[Union[str, Sequence[Any]]], max_new_tokens: int = 128, system: Optional[str] = None,
                           eos_token_id=None, pad_token_id: Optional[int] = None, device: Optional[str] = None) -> List[str]:
    """Several greedy requests as ONE padded batch (server.py:171-290 serves concurrent requests; here they share every pass over the
    weights: `vila_llm_decode_step_batch`, up to 16 rows).  Each prompt is tokenised on its own, rows are right-padded, the images of all
    prompts are encoded by one tower call and consumed in row order (`_embed`, llava_arch.py:454-466).  Returns one decoded reply per prompt."""
    if not prompts:
        return []
    cfg = model.cfg
    dev = device or str(model.device)
    rows, tiles, blocks = [], [], []
    for prompt in prompts:
        text, t, mc = prepare_prompt(prompt, cfg)             # per request, like generate_content: one image -> its tiles
        rows.append(encode_with_images(tokenizer, prompt_text(tokenizer, text, system), cfg.image_token_id))
        tiles.extend(t)
        blocks.extend(mc.get("image", {}).get("block_sizes", [None] * len(t)))
    eos = _eos_of(tokenizer, eos_token_id)
    stop = _eos_set(eos)
    pad = pad_token_id if pad_token_id is not None else (getattr(tokenizer, "pad_token_id", None) or 0)
    L = max(int(r.numel()) for r in rows)
    ids = torch.full((len(rows), L), int(pad), dtype=torch.int64)
    mask = torch.zeros((len(rows), L), dtype=torch.bool)
    for b, r in enumerate(rows):
        ids[b, : r.numel()] = r
        mask[b, : r.numel()] = True
    media = {"image": [t.to(device=dev, dtype=torch.bfloat16) for t in tiles]}
    media_config = {"image": {"block_sizes": blocks}} if any(b is not None for b in blocks) else {}
    out = model.generate(input_ids=ids.to(dev), media=media, media_config=media_config, attention_mask=mask.to(dev), max_new_tokens=max_new_tokens,
                         eos_token_id=eos, pad_token_id=int(pad))
    replies = []
    for row in out.tolist():
        toks = row
        for k, t in enumerate(row):
            if t in stop:
                toks = row[:k]
                break
        replies.append(tokenizer.decode(toks, skip_special_tokens=True).strip())
    return replies


class RequestBatcher:
    """Groups greedy requests that arrive within `window_s` of each other (at most `max_batch` <= 16) into one `generate_content_batch` call.
    `submit` returns a `concurrent.futures.Future` of the reply; one worker thread owns the model.  Requests with different `max_new_tokens`
    or system prompts do not share a batch (the batch runs to the longest reply; a row that stops early is padded like HF does)."""

    def __init__(self, model, tokenizer, window_s: float = 0.005, max_batch: int = 16, run=None):
        import queue
        import threading
        self.model, self.tokenizer, self.window_s, self.max_batch = model, tokenizer, float(window_s), int(max(1, min(16, max_batch)))
        self._run = run or (lambda prompts, n, system: generate_content_batch(self.model, self.tokenizer, prompts, max_new_tokens=n, system=system))
        self._q: "queue.Queue" = queue.Queue()
        self.batches: List[int] = []                     # sizes of the batches that ran (observability / tests)
        self.model_lock = threading.Lock()               # whoever drives the model outside the worker (sampled requests) holds this
        self._stop = False
        self._thread = threading.Thread(target=self._loop, daemon=True)
        self._thread.start()

    def submit(self, prompt, max_new_tokens: int = 128, system: Optional[str] = None):
        from concurrent.futures import Future
        f: Future = Future()
        self._q.put((prompt, int(max_new_tokens), system, f))
        return f

    def close(self):
        self._stop = True
        self._q.put(None)
        self._thread.join(timeout=5)

    def _loop(self):
        import queue
        held = None
        while not self._stop:
            item = held if held is not None else self._q.get()
            held = None
            if item is None:
                break
            group = [item]
            deadline = time.time() + self.window_s
            while len(group) < self.max_batch:
                try:
                    nxt = self._q.get(timeout=max(0.0, deadline - time.time()))
                except queue.Empty:
                    break
                if nxt is None:
                    self._stop = True
                    break
                if nxt[1] != item[1] or nxt[2] != item[2]:           # other generation settings: it starts the next group
                    held = nxt
                    break
                group.append(nxt)
            try:
                with self.model_lock, torch.inference_mode():
                    replies = self._run([g[0] for g in group], item[1], item[2])
                self.batches.append(len(group))
                for g, r in zip(group, replies):
                    g[3].set_result(r)
            except Exception as e:                                    # every waiter of the group sees the failure
                for g in group:
                    g[3].set_exception(e)


class HipBatchEngine:
    """The model side of `ContinuousBatcher`: KV slots of ONE open batched-decode session (`HipQwen2ForCausalLM.batch_open`), driven by
    the batcher's worker thread only.  sampling=True opens the session with per-row sampling (`batch_open(sampling=True)`): `admit` then takes
    a row's (temperature, top_k, top_p, seed) and a `ContinuousBatcher(batch_sampled=True)` puts sampled requests into rows.
    max_ctx: positions per KV slot, up to 32768 (default 2048); `fits` admits what fits the slot, everything longer runs solo.
    share_prefix=True opens the session with a prefix slot (`batch_open(shared_prefix=True)`): requests over the same media — a request's prefix is
    its prompt up to and including its last media placeholder — can then share the K/V of that prefix (`prepare`, `pinned_key`, `pin`, `embed_tail`,
    `admit(..., share=True)`), which a `ContinuousBatcher(share_prefix=True)` drives.  min_shared_len (default 2048): a prefix whose shared length would
    be shorter is not pinned and its request takes an ordinary row — the prefix step's three attention launches cost more than they save on a short
    prefix (a one-tile image, about 256 keys: 1.07 - 1.19x the ordinary step; `DESIGN.md` 4.3b).  A prefix that may be pinned must also fit a slot
    with something behind it, so share_prefix needs max_ctx > min_shared_len: the default 2048 / 2048 pair could never share and is refused.
    penalties=True opens the session with per-row repetition / presence / frequency penalties (`batch_open(penalties=True)`): `admit` then takes a
    row's (rep, pres, freq) and a `ContinuousBatcher(penalties=True)` puts penalised requests into rows.
    logprobs=True opens the session with per-row logprob records (`batch_open(logprobs=True)`): every step records the raw log-probability of each
    row's token and of its 20 most likely alternatives, `read_logprobs` turns a row's records into OpenAI-layout entries, and a
    `ContinuousBatcher(logprobs=True)` puts requests that ask for logprobs into rows.
    constraints=True opens the session with a token automaton per row (`batch_open(constraints=True, max_states=, max_classes=)`: a table of
    max_states x max_classes entries per row): `compile_constraint` turns a request's `response_format` / `guided_choice` / `guided_regex` into an
    automaton (cached per vocabulary), `admit` takes it, and a `ContinuousBatcher(constraints=True)` puts such requests into rows.  compiler: the
    `ConstraintCompiler` to use in place of the one derived from a byte-level BPE tokenizer.
    any_top_k=True (with sampling=True) opens the session with `batch_open(any_top_k=True)`: a sampled row may then carry any top_k >= 0 (0 = no
    top-k filter, i.e. pure top-p sampling; k > 64), and a `ContinuousBatcher(batch_sampled=True, any_top_k=True)` puts such requests into rows.
    adapters=bank (a `vila_amd.lora_serving.AdapterBank`) opens the session with `batch_open(adapters=bank)`: `admit(..., adapter=name)` prefills the
    request under that LoRA adapter, unmerged, and its row steps under it; `embed(..., adapter=name)` encodes the media through the adapter's tuned
    projector where it has one.  A `ContinuousBatcher(adapters=True)` routes requests by their `model` field.  Not with share_prefix."""

    def __init__(self, model, tokenizer, n_slots: int = 8, max_ctx: int = 2048, max_new_tokens: int = 1024, eos_token_id=None,
                 sampling: bool = False, share_prefix: bool = False, min_shared_len: int = 2048, penalties: bool = False, logprobs: bool = False,
                 constraints: bool = False, max_states: int = 512, max_classes: int = 4096, compiler=None, any_top_k: bool = False, adapters=None):
        self.model, self.tokenizer = model, tokenizer
        self.adapters = adapters                            # batch_open(adapters=bank): `admit` takes the name of a row's adapter
        if adapters is not None and share_prefix:
            raise ValueError("HipBatchEngine: adapters= is not served together with share_prefix (the step with adapters has no shared-prefix form)")
        self.sampling = bool(sampling)
        self.any_top_k = bool(any_top_k) and self.sampling  # batch_open(any_top_k=True): a sampled row's top_k may be 0 or above 64
        self.constraints = bool(constraints)                # batch_open(constraints=True, max_states=, max_classes=): `admit` takes a row's automaton
        self.max_states, self.max_classes = int(max_states), int(max_classes)
        self.compiler = compiler                            # a `ConstraintCompiler` (for a tokenizer that is not byte-level BPE); default: the tokenizer's
        self.logprobs = bool(logprobs)                      # batch_open(logprobs=True): every row's steps leave records for `read_logprobs`
        self.penalties = bool(penalties)                    # batch_open(penalties=True): `admit` takes a row's (rep, pres, freq)
        self.share_prefix = bool(share_prefix)
        self.min_shared_len = int(min_shared_len)
        if self.share_prefix and int(max_ctx) <= max(self.min_shared_len, 256):
            raise ValueError(f"HipBatchEngine(share_prefix=True): a prefix is pinned from min_shared_len = {max(self.min_shared_len, 256)} shared positions on and "
                             f"has to fit a slot with its tail and reply behind it; max_ctx = {int(max_ctx)} leaves nothing to share (raise max_ctx, e.g. "
                             "4096 for a dynamic_s2 document, or lower min_shared_len)")
        self._pinned = None                                 # the session's prefix: its key, S, and its embedding rows S .. prefix rows - 1
        self.n_slots, self.max_ctx, self.max_new_tokens = int(n_slots), int(max_ctx), int(max_new_tokens)
        self.eos = _eos_set(_eos_of(tokenizer, eos_token_id))
        self.st = None

    def _session(self):
        llm = self.model.llm
        if self.st is None or getattr(llm, "_bdecode", None) is not self.st:       # first use, or the weights moved and the session was dropped
            kw = dict(sampling=True) if self.sampling else {}
            if self.any_top_k:
                kw["any_top_k"] = True
            if self.share_prefix:
                kw["shared_prefix"] = True
                self._pinned = None                                                 # a new session holds no prefix
            if self.penalties:
                kw["penalties"] = True
            if self.logprobs:
                kw["logprobs"] = True
            if self.constraints:
                kw.update(constraints=True, max_states=self.max_states, max_classes=self.max_classes)
            if self.adapters is not None:
                kw["adapters"] = self.adapters
            self.st = llm.batch_open(self.n_slots, self.max_ctx, self.max_new_tokens, **kw)
        return self.st

    @property
    def shares_prefix(self) -> bool:
        """Whether requests over the same media can share their prefix's K/V in this engine's batch."""
        return self.share_prefix

    def prepare(self, prompt, system):
        """The host side of a request, done ONCE per request and handed on to `embed`, `pin` and `embed_tail`: media loaded and tiled, the prompt's
        token ids, and the key of its prefix — the ids up to and including its last media placeholder plus a digest of the media bytes; None for a
        request without media.  No tower, no projector."""
        import hashlib
        cfg = self.model.cfg
        text, tiles, media_config = prepare_prompt(prompt, cfg)
        ids = encode_with_images(self.tokenizer, prompt_text(self.tokenizer, text, system), cfg.image_token_id)
        at = (ids == cfg.image_token_id).nonzero()
        key, n_tail = None, 0
        if at.numel() and tiles:
            h = hashlib.sha1()
            for t in tiles:
                t = t.detach().cpu().contiguous()
                h.update(str((tuple(t.shape), str(t.dtype))).encode())
                h.update(t.view(torch.uint8).numpy().tobytes())
            key, n_tail = (tuple(ids[:int(at[-1]) + 1].tolist()), h.hexdigest()), int(ids.numel()) - int(at[-1]) - 1
        return SimpleNamespace(ids=ids, tiles=tiles, media_config=media_config, key=key, n_tail=n_tail)

    @property
    def pinned_key(self):
        """The key of the prefix this engine's session holds, or None: none was pinned, or the session that held it is gone (the weights moved, the
        llm opened another batch session)."""
        if self.st is None or getattr(self.model.llm, "_bdecode", None) is not self.st:
            self._pinned = None
        return None if self._pinned is None else self._pinned.key

    def pin(self, e, prep) -> bool:
        """Make the prefix of the request (e = `embed` of it, prep = `prepare` of it) the session's shared prefix: the whole prompt is prefilled into the
        prefix slot once, and its rows up to the last whole 256-position chunk of the prefix become the shared keys.  True: `admit(e, share=True)`
        then takes the request without another prefill.  Only while no live row shares the current prefix, and only for a request that `fits`.
        False, with the session's prefix left as it was: the shared length would be below min_shared_len, or the prompt does not fit a slot."""
        rows = int(e.shape[0]) - prep.n_tail                                       # embedding rows up to the end of the last media item
        if prep.key is None or rows // 256 * 256 < max(self.min_shared_len, 256) or int(e.shape[0]) + 1 > self.max_ctx:
            return False
        st = self._session()
        self._pinned = None
        S = self.model.llm.batch_set_prefix(st, e, prefix_len=rows)
        self._pinned = SimpleNamespace(key=prep.key, S=S, rest=e[S:rows].clone())
        return True

    def embed_tail(self, prep):
        """A request whose key is `pinned_key` -> (its embeddings from row S on, S): the pinned prefix's rows behind the last whole chunk, then the
        text behind the last media placeholder, embedded the way `ChatSession.ask` embeds a new turn.  No tower, no projector."""
        pin = self._pinned
        tail = prep.ids[prep.ids.numel() - prep.n_tail:].to(pin.rest.device)
        e = self.model.llm.embed_tokens(tail[None])[0].to(pin.rest.dtype) if tail.numel() else pin.rest[:0]
        return torch.cat([pin.rest, e], 0), pin.S

    @property
    def batches_sampled(self) -> bool:
        """Whether a sampled request (top_k in 1..64) can take a row of this engine's batch."""
        return self.sampling

    @property
    def batches_any_top_k(self) -> bool:
        """Whether a sampled request with top_k = 0 (no top-k filter) or top_k > 64 can take a row of this engine's batch."""
        return self.any_top_k

    @property
    def batches_penalties(self) -> bool:
        """Whether a request with repetition / presence / frequency penalties can take a row of this engine's batch."""
        return self.penalties

    @property
    def batches_logprobs(self) -> bool:
        """Whether a request that asks for logprobs can take a row of this engine's batch."""
        return self.logprobs

    @property
    def batches_constraints(self) -> bool:
        """Whether a request with `response_format` / `guided_choice` / `guided_regex` can take a row of this engine's batch."""
        return self.constraints

    @property
    def batches_adapters(self) -> bool:
        """Whether a request under a LoRA adapter of the engine's bank can take a row of this engine's batch."""
        return self.adapters is not None

    def has_adapter(self, name) -> bool:
        """Whether `name` is an adapter loaded into the engine's bank."""
        return self.adapters is not None and name in self.adapters

    def compile_constraint(self, asks):
        """The automaton of a request's structured-output fields (`structured_of`), compiled for this engine's vocabulary within its rows' table; a
        ValueError where the schema or pattern is not served, the vocabulary cannot spell it, or it does not fit."""
        comp = self.compiler
        if comp is None:
            comp = constraint_compiler(self.tokenizer, self.model.cfg.llm.vocab_size, sorted(self.eos), max_table=self.max_states * self.max_classes,
                                       max_classes=self.max_classes)
        return constraint_of(asks, comp)

    def read_logprobs(self, slot: int, toks: Sequence[int], top_logprobs: int) -> List[Dict[str, Any]]:
        """The OpenAI-layout entries (`logprob_entries`) of the reply tokens `toks` of the request in row `slot`: its first token's record and those
        of its steps (`llm.batch_logprobs`), cut where `toks` is cut.  Before the row is released."""
        lp = self.model.llm.batch_logprobs(self._session(), slot)
        return logprob_entries(self.tokenizer, toks, lp.token_logprobs, lp.top_logprobs, lp.top_ids, int(top_logprobs))

    def fresh_seed(self) -> int:
        """The seed of a sampled request that names none, derived as `generate` derives it."""
        return self.model.llm._fresh_seed()

    def fits(self, n_prompt_tokens: int, max_new_tokens: int) -> bool:
        return max_new_tokens <= self.max_new_tokens and n_prompt_tokens + max_new_tokens <= self.max_ctx

    def embed(self, prompt, system, prep=None, adapter=None):
        """Prompt -> spliced embeddings [S, H] on the device (tower + projector + splice run here, on the worker thread).  prep: what `prepare`
        returned for this request, so that its media is not loaded and tiled again.  adapter: the request's adapter, whose tuned projector (if it
        keeps one) encodes the media."""
        cfg = self.model.cfg
        dev = str(self.model.device)
        if prep is None:
            text, tiles, media_config = prepare_prompt(prompt, cfg)
            ids = encode_with_images(self.tokenizer, prompt_text(self.tokenizer, text, system), cfg.image_token_id)
        else:
            ids, tiles, media_config = prep.ids, prep.tiles, prep.media_config
        media = {"image": [t.to(device=dev, dtype=torch.bfloat16) for t in tiles]}
        e, _, _ = self.model._embed(ids[None].to(dev), media, media_config, **({} if adapter is None else dict(adapter=adapter, adapters=self.adapters)))
        return e[0]

    def admit(self, slot: int, embeds, sampling=None, share: bool = False, first_row: int = 0, penalties=None, constraint=None, adapter=None) -> int:
        kw = {} if sampling is None else dict(sampling=sampling)
        if adapter is not None:
            kw.update(adapter=adapter)
        if constraint is not None:
            kw.update(constraint=constraint)
        if share:
            kw.update(share=True, first_row=first_row)
        if penalties is not None:
            kw.update(penalties=penalties)
        return self.model.llm.batch_admit(self._session(), slot, embeds, **kw)

    def run(self, k: int) -> None:
        self.model.llm.batch_run(self._session(), k)

    def read(self):
        st = self._session()
        n = st.n_out.tolist()
        top = max(max(n), 1)
        return n, st.out_ids[:, :min(top, st.out_ids.shape[1])].tolist()

    def release(self, slots) -> None:
        self.model.llm.batch_release(self._session(), slots)

    def solo(self, prompt, max_new_tokens, system, streamer=None, **gen) -> str:
        return generate_content(self.model, self.tokenizer, prompt, max_new_tokens=max_new_tokens, system=system, streamer=streamer, **gen)

    def decode(self, toks) -> str:
        return self.tokenizer.decode(toks, skip_special_tokens=True).strip()


class ContinuousBatcher:
    """Continuous batching in front of the batched decode step (the reference's server answers requests as they arrive,
    server.py:171-290).  ONE worker thread owns the model (every request — greedy, sampled, batched or not — is executed by
    it, so no two threads ever drive the sessions, the staging buffers or the captured graphs).  Between chunks of <= `chunk` decode steps the
    worker admits waiting greedy requests into free rows (each newcomer is prefilled alone into its KV slot and joins the next step), retires
    rows at EOS / max_new_tokens and hands their slot to the next request — a request that arrives one step after a batch started waits for at
    most one chunk, not for the whole batch.  Requests the batched step cannot serve (sampling, replies or prompts beyond the slots' cache) run
    solo on the same thread once the live rows have drained; arrival order is kept (a solo request at the head blocks later admissions).
    batch_sampled=True (opt-in; needs an engine whose `batches_sampled` is true, i.e. `HipBatchEngine(sampling=True)`): a request with
    temperature > 0 and top_k (default 50) in 1..64 takes a free row like a greedy one — the reference's default request (0.2 / 0.9) then
    batches instead of stalling the line.  The trade: the batched step sums in another order than the solo step, so the ids of a sampled
    request are no longer those of its solo run (same distribution, same seed -> same reply within the batched path).  A request without a
    seed gets one derived as `generate` derives it.  top_k = 0 or > 64 stays solo, unless:
    any_top_k=True (opt-in, with batch_sampled; needs an engine whose `batches_any_top_k` is true, i.e. `HipBatchEngine(sampling=True,
    any_top_k=True)`): a sampled request with ANY top_k >= 0 takes a row — top_k = 0, no top-k filter, is how an OpenAI-style client samples
    (temperature + top_p), and without the flag one such request at the head of the line waits for the live rows to drain and blocks later
    admissions.  Its row is drawn on the device by the solo sampler's exact path.
    share_prefix=True (opt-in; needs an engine whose `shares_prefix` is true, i.e. `HipBatchEngine(share_prefix=True)`): requests over the same
    media share the K/V of their common prefix.  When no live row shares the current prefix, a request with media that fits a slot PINS its own
    (`engine.pin`: one tower / projector / prefill run); later requests with the same key (`engine.prepare(...).key == engine.pinned_key`) are
    admitted as sharing rows, for which only the text behind the media is embedded and prefilled.  A request without media, with a prefix the engine finds too short to pay, or with another key
    while sharers live, takes an ordinary row and does not wait; the pin moves once the sharers have retired.  `events` records ("pin", slot) and ("share", slot).
    penalties=True (opt-in; needs an engine whose `batches_penalties` is true, i.e. `HipBatchEngine(penalties=True)`): a request with a non-neutral
    repetition_penalty / presence_penalty / frequency_penalty that is otherwise batchable takes a row, whose counts start from zero.  Without the
    flag such a request runs solo, the way a sampled one does without batch_sampled.  A request with neutral values is served exactly as before.
    logprobs=True (opt-in; needs an engine whose `batches_logprobs` is true, i.e. `HipBatchEngine(logprobs=True)`): a request submitted with
    logprobs=True (and top_logprobs=k) that is otherwise batchable takes a row, and its future resolves to a `ReplyWithLogprobs` whose entries come
    from the row's records (`engine.read_logprobs`).  Without the flag such a request runs solo (`engine.solo` gets the two keywords), exactly as
    `penalties=` does it.  A request that does not ask is served exactly as before.
    constraints=True (opt-in; needs an engine whose `batches_constraints` is true, i.e. `HipBatchEngine(constraints=True)`): a request submitted
    with `response_format`, `guided_choice` or `guided_regex` that is otherwise batchable takes a row: its automaton is compiled on the worker thread
    (`engine.compile_constraint`; a compile error fails that request alone) and handed to `engine.admit`.  Without the flag such a request runs solo
    (`engine.solo` gets the field).  With a `stream` it is refused.  A request that does not ask is served exactly as before.
    adapters=True (opt-in; needs an engine whose `batches_adapters` is true, i.e. `HipBatchEngine(adapters=bank)`): a request submitted with
    model=name, name an adapter loaded into the engine's bank (`engine.has_adapter`), takes a row under that adapter, unmerged — vLLM's convention
    for its `model` field; requests under different adapters and base requests share every step.  Any other `model` value, and every `model` value
    without the flag, is dropped: the request is the base model's, served exactly as before.  A request under an adapter never runs solo (a solo
    run would need a second session, which evicts the batcher's): one the session cannot take as a row — it samples without batch_sampled, asks
    for penalties, logprobs or structured output without that flag, or does not fit a slot — fails with a ValueError that names what is missing."""

    def __init__(self, engine, max_batch: int = 8, chunk: int = 8, batch_sampled: bool = False, share_prefix: bool = False, penalties: bool = False,
                 logprobs: bool = False, constraints: bool = False, any_top_k: bool = False, adapters: bool = False):
        import queue
        import threading
        self.engine = engine
        self.adapters = bool(adapters) and bool(getattr(engine, "batches_adapters", False))
        self.batch_sampled = bool(batch_sampled) and bool(getattr(engine, "batches_sampled", False))
        self.any_top_k = bool(any_top_k) and self.batch_sampled and bool(getattr(engine, "batches_any_top_k", False))
        self.penalties = bool(penalties) and bool(getattr(engine, "batches_penalties", False))
        self.logprobs = bool(logprobs) and bool(getattr(engine, "batches_logprobs", False))
        self.constraints = bool(constraints) and bool(getattr(engine, "batches_constraints", False))
        self.share_prefix = bool(share_prefix) and bool(getattr(engine, "shares_prefix", False))
        self._pin_rows = set()                           # the live rows that share the engine's current prefix (`engine.pinned_key`)
        self._seedless = 0
        self.max_batch = int(max(1, min(16, max_batch, getattr(engine, "n_slots", max_batch))))
        self.chunk = int(max(1, chunk))
        self._q: "queue.Queue" = queue.Queue()
        self.events: List[tuple] = []                    # ("admit" | "retire" | "solo" | "run", ...) — observability / tests
        self.thread_ids = set()
        self._stop = False
        self.dead: Optional[BaseException] = None        # set (BEFORE the queue is drained) when the worker thread has died
        self._thread = threading.Thread(target=self._loop, daemon=True)
        self._thread.start()

    def submit(self, prompt, max_new_tokens: int = 128, system: Optional[str] = None, stream: Optional["TextStream"] = None, **gen):
        """-> Future of the decoded reply.  gen: temperature / top_p / top_k / seed — a request with temperature > 0 is a solo one, unless the
        batcher was built with batch_sampled=True and the request's top_k lies in 1..64 (with any_top_k=True: is >= 0); then it takes a row.
        stream: a `TextStream` that receives the request's tokens while the row is still decoding — its first token at admission, then
        the new ones after every chunk of steps (server.py:241-270 streams a reply as it is generated); `end()` when the row retires,
        `fail()` with the exception the future gets."""
        from concurrent.futures import Future
        f: Future = Future()
        if "model" in gen:                                                 # (only a loaded adapter's name routes; anything else is the base model)
            name = gen.pop("model")
            if self.adapters and name is not None and self.engine.has_adapter(name):
                gen["adapter"] = name
        req = SimpleNamespace(prompt=prompt, max_new=int(max_new_tokens), system=system, gen=gen, fut=f, stream=stream)
        try:
            _logprobs_of(gen.get("logprobs"), gen.get("top_logprobs"))     # a bad pair fails the request here, not after its row has run
            check_structured_request(gen, stream is not None)              # ... and so do two structured-output fields, or one with a stream
        except ValueError as ex:
            self._fail(req, ex)
            return f
        if self.dead is not None:
            self._fail(req, self.dead)
            return f
        self._q.put(req)
        # the worker may have died between the check above and the put — it sets `dead` BEFORE it drains the queue, so a request
        # that slipped in behind the drain sees `dead` here and fails now instead of waiting in a queue nobody reads (a request the drain did
        # reach is failed there; failing a future / stream twice is harmless: `_fail` ignores the second)
        if self.dead is not None:
            self._fail(req, self.dead)
        return f

    def close(self):
        self._stop = True
        self._q.put(None)
        self._thread.join(timeout=10)

    @staticmethod
    def _greedy(req) -> bool:
        t = req.gen.get("temperature")
        return not t or t <= 0

    def _row_sampling(self, req):
        """(temperature, top_k, top_p, seed) when the request samples AND the batched sampler serves it, else None."""
        if not self.batch_sampled or self._greedy(req):
            return None
        g = req.gen
        top_k = 50 if g.get("top_k") is None else int(g["top_k"])
        if not (1 <= top_k <= 64 or (self.any_top_k and top_k >= 0)):
            return None
        seed = g.get("seed")
        if seed is None:                                               # once per request: kept in `gen`, so a retry of the admission re-uses it
            fresh = getattr(self.engine, "fresh_seed", None)
            if callable(fresh):
                seed = int(fresh())
            else:
                self._seedless += 1
                seed = (torch.initial_seed() + 0x9E3779B97F4A7C15 * self._seedless) & 0xFFFFFFFFFFFFFFFF
            req.gen = dict(g, seed=seed)
        return (float(g["temperature"]), top_k, 1.0 if g.get("top_p") is None else float(g["top_p"]), int(seed))

    @staticmethod
    def _row_penalties(req):
        """(rep, pres, freq) of a request that asks for a non-neutral penalty, else None."""
        pen = _penalties_of(req.gen)
        return tuple(pen.get(k, v) for k, v in PENALTY_NEUTRAL.items()) if pen else None

    @staticmethod
    def _row_logprobs(req) -> Optional[int]:
        """The number of alternatives per token of a request that asks for logprobs, else None."""
        return _logprobs_of(req.gen.get("logprobs"), req.gen.get("top_logprobs"))

    def _row_constraint(self, req):
        """The automaton of a request that asks for structured output (compiled by the engine, on the worker thread), else None."""
        asks = structured_of(req.gen)
        return self.engine.compile_constraint(asks) if asks else None

    def _batchable(self, req) -> bool:
        if not self.constraints and structured_of(req.gen):
            return False                                                # a constrained request without the flag runs solo
        if not self.penalties and self._row_penalties(req) is not None:
            return False                                                # a penalised request without the flag runs solo
        if not self.logprobs and req.gen.get("logprobs"):
            return False                                                # ... and so does one that asks for logprobs
        return self._greedy(req) or self._row_sampling(req) is not None

    def _adapter_refusal(self, req) -> Optional[str]:
        """Why a request under an adapter cannot take a row of this batcher's session (it never runs solo), or None."""
        what = None
        if structured_of(req.gen) and not self.constraints:
            what = "structured output needs create_app(constraints=True) / ContinuousBatcher(constraints=True)"
        elif self._row_penalties(req) is not None and not self.penalties:
            what = "penalties need create_app(penalties=True) / ContinuousBatcher(penalties=True)"
        elif req.gen.get("logprobs") and not self.logprobs:
            what = "logprobs need create_app(logprobs=True) / ContinuousBatcher(logprobs=True)"
        elif not self._greedy(req) and not self.batch_sampled:
            what = "a sampled request (temperature > 0) needs create_app(batch_sampled=True) / ContinuousBatcher(batch_sampled=True)"
        elif not self._greedy(req) and self._row_sampling(req) is None:
            what = "top_k = 0 or > 64 needs create_app(any_top_k=True) / ContinuousBatcher(any_top_k=True)"
        if what is None:
            return None
        return f"a request under the adapter '{req.gen['adapter']}' is served as a row of the batched session only, and {what}"

    @staticmethod
    def _fail(req, ex) -> None:
        if getattr(req, "_failed", False):               # (a dying worker's drain and `submit`'s re-check may both reach a request)
            return
        req._failed = True
        if not req.fut.done():
            req.fut.set_exception(ex)
        if getattr(req, "stream", None) is not None:
            req.stream.fail(ex)

    def _emit(self, row, new) -> None:
        """A row's new tokens -> its stream, like HF's `streamer.put` per token: up to AND including the first EOS, never past max_new_tokens."""
        st = row.req.stream
        if st is None or row.closed:
            return
        for t in new:
            if row.sent >= row.req.max_new:
                break
            st.put([t])
            row.sent += 1
            if t in self.engine.eos:
                row.closed = True
                break

    def _finish(self, row, toks, slot=None):
        eng = self.engine
        for k, t in enumerate(toks):                       # HF stops AFTER emitting eos; decode(skip_special_tokens) drops it
            if t in eng.eos:
                toks = toks[:k]
                break
        text = eng.decode(toks)
        if row.req.gen.get("logprobs"):                    # (the row is still live: its records are read before it is released)
            text = ReplyWithLogprobs(text, eng.read_logprobs(slot, toks, self._row_logprobs(row.req)))
        row.req.fut.set_result(text)
        if row.req.stream is not None:
            row.req.stream.end()

    def _embed_for(self, req, slot):
        """A request's embeddings for `slot` and how to admit them: (embeds, prompt positions, admit keywords).  Without share_prefix: the whole
        prompt, an ordinary row.  With it the request is prepared once (media, ids, key) and is: a sharing row when its key is the one the engine
        holds; the pin itself when no live row shares the current prefix, the request fits a slot and the engine finds the prefix worth pinning;
        an ordinary row otherwise.  What does not fit is decided before anything is pinned: the caller then sends it solo, as ever."""
        eng = self.engine
        if req.gen.get("adapter") is not None:                         # (an engine with adapters shares no prefix)
            e = eng.embed(req.prompt, req.system, adapter=req.gen["adapter"])
            return e, int(e.shape[0]), dict(adapter=req.gen["adapter"])
        if not self.share_prefix:
            e = eng.embed(req.prompt, req.system)
            return e, int(e.shape[0]), {}
        prep = eng.prepare(req.prompt, req.system)
        if prep.key is not None and prep.key == eng.pinned_key:
            e, first_row = eng.embed_tail(prep)
            self.events.append(("share", slot))
            return e, first_row + int(e.shape[0]), dict(share=True, first_row=first_row)
        e = eng.embed(req.prompt, req.system, prep)
        n = int(e.shape[0])
        if prep.key is not None and not self._pin_rows and req.max_new >= 1 and eng.fits(n, req.max_new) and eng.pin(e, prep):
            self.events.append(("pin", slot))
            return e, n, dict(share=True)
        return e, n, {}

    def _loop(self):
        """The worker: `_loop_body` under a guard — if the worker dies, everything it held and everything still queued fails with the
        cause instead of hanging (the futures / streams of a dead worker would never resolve)."""
        import collections
        import queue
        pending = collections.deque()
        rows: Dict[int, Any] = {}
        try:
            self._loop_body(pending, rows)
        except BaseException as ex:                                    # noqa: BLE001 — the thread is going away either way
            self._stop = True
            err = RuntimeError(f"batcher worker died: {ex!r}")
            self.dead = err                                             # first: `submit` re-checks it behind its put (see there)
            for r in list(rows.values()):
                self._fail(r.req, err)
            for p in pending:
                self._fail(p, err)
            while True:
                try:
                    item = self._q.get(block=False)
                except queue.Empty:
                    break
                if item is not None:
                    self._fail(item, err)

    def _loop_body(self, pending, rows):
        import queue
        import threading
        self.thread_ids.add(threading.get_ident())
        eng = self.engine
        free = list(range(self.max_batch))
        steps = 0
        with torch.inference_mode():
            while True:
                # ---- take what has arrived (block only when there is nothing to do) ----
                while True:
                    try:
                        item = self._q.get(block=not rows and not pending)
                    except queue.Empty:
                        break
                    if item is None:
                        self._stop = True
                        break
                    pending.append(item)
                if self._stop:
                    for r in list(rows.values()) + [SimpleNamespace(req=p) for p in pending]:
                        if not r.req.fut.done():
                            self._fail(r.req, RuntimeError("batcher closed"))
                    return
                # ---- admit greedy requests at the head of the line into free rows; a solo request waits for the rows to drain ----
                while pending and free:
                    req = pending[0]
                    slot = None                                        # the KV slot this admission took, if it got that far
                    try:
                        under = req.gen.get("adapter")                 # a request under an adapter takes a row or fails: it never runs solo
                        if under is not None and self._adapter_refusal(req) is not None:
                            raise ValueError(self._adapter_refusal(req))
                        if not self._batchable(req) or req.gen.get("_solo"):
                            break
                        e, n_prompt, how = self._embed_for(req, free[0])
                        if not eng.fits(n_prompt, req.max_new) or req.max_new < 1:
                            if under is not None:
                                raise ValueError(f"a request under the adapter '{under}' is served as a row of the batched session only, and its "
                                                 f"{n_prompt} prompt positions + {req.max_new} new tokens do not fit a slot (create_app(max_ctx=))")
                            req.gen = dict(req.gen, _solo=True)
                            break
                        pending.popleft()
                        slot = free.pop(0)
                        sampling = self._row_sampling(req)
                        pen = self._row_penalties(req)
                        if pen is not None:                            # (keyword only when asked for: a neutral request makes the call it always made)
                            how = dict(how, penalties=pen)
                        con = self._row_constraint(req)
                        if con is not None:                            # (likewise)
                            how = dict(how, constraint=con)
                        first = eng.admit(slot, e, **how) if sampling is None else eng.admit(slot, e, sampling, **how)
                        if pen is not None or con is not None or under is not None:
                            how = {k: v for k, v in how.items() if k not in ("penalties", "constraint", "adapter")}
                        if how:
                            self._pin_rows.add(slot)
                        row = SimpleNamespace(req=req, toks=[first], read=0, sent=0, closed=False)
                        self.events.append(("admit", slot, steps, len(rows)))
                        self._emit(row, [first])
                        if first in eng.eos or req.max_new <= 1:
                            self._finish(row, row.toks, slot)
                            eng.release([slot])
                            free.append(slot)
                            self._pin_rows.discard(slot)
                            self.events.append(("retire", slot, steps))
                            slot = None
                        else:
                            rows[slot] = row
                            slot = None                                # owned by `rows` from here on
                    except Exception as ex:                            # the request fails, the batch goes on — and the slot goes back
                        if pending and pending[0] is req:
                            pending.popleft()
                        if slot is not None:
                            rows.pop(slot, None)
                            self._pin_rows.discard(slot)
                            try:
                                eng.release([slot])
                            except Exception:
                                pass
                            if slot not in free:
                                free.append(slot)
                            self.events.append(("admit_failed", slot, steps))
                        self._fail(req, ex)
                if not rows:
                    if pending and (not self._batchable(pending[0]) or pending[0].gen.get("_solo")):
                        req = pending.popleft()
                        gen = {k: v for k, v in req.gen.items() if k != "_solo" and v is not None}
                        self.events.append(("solo", steps))
                        try:
                            if req.stream is not None:
                                gen["streamer"] = req.stream
                            text = eng.solo(req.prompt, req.max_new, req.system, **gen)
                            req.fut.set_result(text)
                            if req.stream is not None:
                                req.stream.finish(text)                 # (an engine whose generate took no streamer)
                        except Exception as ex:
                            self._fail(req, ex)
                    continue
                # ---- one chunk of batched steps: never past the row that is closest to its max_new_tokens ----
                k = min(self.chunk, min(r.req.max_new - len(r.toks) for r in rows.values()))
                try:
                    eng.run(k)
                    n_out, out = eng.read()
                except Exception as ex:
                    for r in rows.values():
                        self._fail(r.req, ex)
                    free.extend(rows)
                    rows.clear()
                    self._pin_rows.clear()
                    continue
                steps += k
                self.events.append(("run", k, len(rows)))
                done = []
                for slot, row in rows.items():
                    try:                                               # a tokenizer / stream failure fails THIS request only
                        new = out[slot][row.read:n_out[slot]]
                        row.toks.extend(new)
                        row.read = n_out[slot]
                        self._emit(row, new)
                        if any(t in eng.eos for t in row.toks) or len(row.toks) >= row.req.max_new:
                            self._finish(row, row.toks[:row.req.max_new], slot)
                            done.append(slot)
                    except Exception as ex:
                        self._fail(row.req, ex)
                        done.append(slot)
                for slot in done:
                    del rows[slot]
                    self._pin_rows.discard(slot)
                    self.events.append(("retire", slot, steps))
                idle = done + free                                     # idle rows took part in the steps too: re-wind them
                eng.release(idle)
                free.extend(done)


_MODELS = None


def _request_models():
    """pydantic request schema (server.py:38-110), built once at module scope so FastAPI can resolve the annotations."""
    global _MODELS
    if _MODELS is None:
        import pydantic
        ChatMessage = pydantic.create_model("ChatMessage", role=(str, ...), content=(Union[str, List[Dict[str, Any]]], ...))
        ChatCompletionRequest = pydantic.create_model(
            "ChatCompletionRequest", model=(str, ...), messages=(List[ChatMessage], ...), max_tokens=(Optional[int], 512),
            temperature=(Optional[float], 0.2), top_p=(Optional[float], 0.9), stream=(Optional[bool], False),      # server.py:101-102
            repetition_penalty=(Optional[float], 1.0), presence_penalty=(Optional[float], 0.0), frequency_penalty=(Optional[float], 0.0),
            logprobs=(Optional[bool], False), top_logprobs=(Optional[int], None),                                  # OpenAI's fields; top_logprobs 0..20
            top_k=(Optional[int], None),                         # HF's / vLLM's field: absent = 50; 0 (HF) or -1 (vLLM) = no top-k filter
            # structured output: the reference's ResponseFormat ({"type": "json_schema", "json_schema": {"schema": ...}}), vLLM's guided fields
            response_format=(Optional[Dict[str, Any]], None), guided_choice=(Optional[List[str]], None), guided_regex=(Optional[str], None))
        _MODELS = (ChatMessage, ChatCompletionRequest)
    return _MODELS


def continuous_batching(model) -> bool:
    """`create_app`'s choice of batcher: `ContinuousBatcher` when the model's LLM has the batched decode step (its `can_batch_decode_step()`:
    a bf16 head-dim-128 decoder, or one quantised with quantize_w4(batch_decode=True)), else the static-window `RequestBatcher`."""
    pred = getattr(getattr(model, "llm", None), "can_batch_decode_step", None)
    return bool(pred()) if callable(pred) else False


def create_app(model, tokenizer, model_name: str = "NVILA-8B", batch_window_s: Optional[float] = None, max_batch: int = 8,
               stream_timeout_s: Optional[float] = 600.0, batch_sampled: bool = False, max_ctx: int = 2048,
               prompt_lookup_num_tokens: Optional[int] = None, spec_sample: bool = False, share_prefix: bool = False, penalties: bool = False,
               logprobs: bool = False, constraints: bool = False, any_top_k: bool = False, spec_processed: bool = False, adapters=None,
               max_adapters: int = 4):
    """FastAPI app with the reference's POST /chat/completions (server.py:171-290).  Import-time optional: needs fastapi + pydantic.
    batch_window_s: when set (any value), requests go through a batcher whose ONE worker thread owns the model: `ContinuousBatcher` (greedy
    requests join / leave the batched decode step between steps; sampled ones run solo on the same thread) where the model has the batched
    step, else `RequestBatcher` (greedy requests that arrive within the window share a batch; the rest run under the batcher's lock).
    batch_sampled=True (with a ContinuousBatcher only): sampled requests — the default request, temperature 0.2 / top_p 0.9 / top_k 50 — join
    the batched step as rows instead of running solo.  The trade: the ids of a sampled request are no longer those of its solo run (the
    batched step sums in another order); greedy requests are served exactly as before.
    max_ctx (ContinuousBatcher only): positions per KV slot of the batched session, up to 32768.  The default 2048 keeps the KV memory as it was;
    a larger value lets long prompts (dynamic_s2's 2304 image tokens, video, multi-image chats) take a row instead of running solo.
    prompt_lookup_num_tokens=k: greedy requests that this app runs solo (not through a batcher) decode speculatively with k lookup drafts per
    step; their replies are the greedy replies.  None (default): every request takes the path it always took.
    spec_sample=True (with prompt_lookup_num_tokens): sampled requests that run solo — the default request — speculate as well when their top_k
    lies in 1..64 (the sampled verify step's range); their replies are those of the same sampled request without drafts.  Other sampled
    requests, and every sampled request without the flag, stay non-speculative.
    share_prefix=True (ContinuousBatcher only; default off): requests over the same media — several questions about one video or document —
    share the K/V of their common prefix in the batched session (`ContinuousBatcher(share_prefix=True)`): the media is encoded and prefilled once,
    and every step reads its keys once for all of them.  Needs max_ctx above the engine's min_shared_len (2048): with the default max_ctx no
    prefix worth sharing fits a slot, and the pairing is refused with a ValueError (`create_app(..., share_prefix=True, max_ctx=4096)` or more).
    The request's repetition_penalty (HF's rule, default 1.0), presence_penalty and frequency_penalty (OpenAI's, default 0.0) reach `llm.generate`;
    a request that leaves them neutral is served exactly as before.  penalties=True (ContinuousBatcher only; default off): the batched session is
    opened with per-row penalties, so a penalised request takes a row; without it such a request runs solo, as a sampled one does without
    batch_sampled.
    The request's `logprobs`: true (with `top_logprobs`: 0..20) adds "logprobs": {"content": [...]} to the response's choice, one OpenAI-layout
    entry per reply token (RAW log-probabilities: the model's own distribution, whatever the request's temperature, top_p and penalties); a request
    without the fields gets today's response byte for byte and makes today's calls.  top_logprobs without logprobs, and logprobs together with
    stream (entries on SSE pieces are not served), come back as the usual 500 body.  logprobs=True (ContinuousBatcher only; default off): the
    batched session records logprobs per row, so such a request takes a row; without it such a request runs solo, as `penalties=` does it.
    The request's `response_format` (the reference's ResponseFormat: {"type": "json_schema", "json_schema": {"schema": ...}}), `guided_choice` (a
    list of strings) or `guided_regex` (a pattern) holds the reply to the schema (laid out as `json.dumps(obj, indent=2)`), to one of the strings or
    to the pattern (`generate_content` has the served subsets; `max_tokens` can still cut the reply).  A request without the fields is served exactly
    as before.  A compile error (`json_object`, an unsupported keyword, a pattern the vocabulary cannot spell), two of the fields at once, and any of
    them together with `stream` come back as the usual 500 body.  constraints=True (ContinuousBatcher only; default off): the batched session holds
    an automaton per row, so such a request takes a row; without it such a request runs solo, as `penalties=` does it.
    The request's `top_k` (optional): absent = 50, today's calls and bits; 0, or vLLM's -1, = no top-k filter (pure temperature / top-p sampling,
    what an OpenAI-style client means); any other negative value comes back as the usual 500 body.  A greedy request ignores it.
    any_top_k=True (default off; with batch_sampled, ContinuousBatcher only): the batched session's sampler serves every top_k >= 0, so a sampled
    request with top_k = 0 or > 64 takes a row; without it such a request runs solo, as a penalised one does without `penalties=`.  With
    spec_sample (and prompt_lookup_num_tokens) it lets solo sampled requests with such a top_k speculate as well.
    spec_processed=True (default off; with prompt_lookup_num_tokens): penalised, logprob and structured requests that this app runs solo speculate
    as well (`generate_content(spec_processed=True)`) instead of dropping the drafts; their replies are those of the same requests without drafts.
    adapters={"name": folder, ...} (default None; needs batch_window_s and a model with the batched step, i.e. the ContinuousBatcher; bf16, not with
    share_prefix): the LoRA adapters of the folders (written by `save_adapter`) are loaded into an `AdapterBank` of max_adapters slots beside the
    untouched base model, and a request whose `model` field names one of them takes a row of the batched session under it, unmerged — vLLM's
    convention; requests under different adapters and base requests share every weight pass.  Any other `model` value is served byte for byte as
    before.  An adapter request that the session cannot take as a row (e.g. a sampled one without batch_sampled) comes back as the usual 500 body
    naming the missing flag; it does not run solo, because a second session would evict the batcher's."""
    bank = None
    if adapters:
        if batch_window_s is None or not continuous_batching(model):
            raise ValueError("create_app(adapters=): adapters are served as rows of the batched session; pass batch_window_s and a model that has the "
                             "batched decode step (bf16, head_dim 128)")
        from .lora_serving import AdapterBank
        ranks = [int(json.load(open(os.path.join(str(f), "adapter_config.json")))["r"]) for f in adapters.values()]
        bank = AdapterBank(model, capacity=max(int(max_adapters), 1), r=max(ranks))
        for name, folder in adapters.items():
            if name == model_name:
                raise ValueError(f"create_app(adapters=): '{name}' is the base model's name")
            bank.load(name, folder)
    from fastapi import FastAPI
    from fastapi.responses import JSONResponse, StreamingResponse

    ChatMessage, ChatCompletionRequest = _request_models()
    app = FastAPI()
    batcher = None
    if batch_window_s is not None:
        if continuous_batching(model):
            # the default call is the one it always was (keywords only when asked for): an engine class substituted for HipBatchEngine with the
            # narrower constructor (model, tokenizer, n_slots), as tests/test_w4_batch_decode_cpu.py does, keeps working
            kw = dict(n_slots=max_batch)
            if int(max_ctx) != 2048:
                kw["max_ctx"] = int(max_ctx)
            if batch_sampled:
                kw["sampling"] = True
            if share_prefix:
                kw["share_prefix"] = True
            if penalties:
                kw["penalties"] = True
            if logprobs:
                kw["logprobs"] = True
            if constraints:
                kw["constraints"] = True
            if any_top_k and batch_sampled:
                kw["any_top_k"] = True
            if bank is not None:
                kw["adapters"] = bank
            engine = HipBatchEngine(model, tokenizer, **kw)
            batcher = ContinuousBatcher(engine, max_batch=max_batch, batch_sampled=batch_sampled, **(dict(share_prefix=True) if share_prefix else {}),
                                        **(dict(penalties=True) if penalties else {}), **(dict(logprobs=True) if logprobs else {}),
                                        **(dict(constraints=True) if constraints else {}),
                                        **(dict(any_top_k=True) if any_top_k and batch_sampled else {}),
                                        **(dict(adapters=True) if bank is not None else {}))
        else:
            batcher = RequestBatcher(model, tokenizer, window_s=batch_window_s)
    app.state.batcher = batcher
    app.state.adapters = bank

    def _prompt_of(messages):
        parts: List[Any] = []
        system = None
        for m in messages:
            if m.role == "system" and isinstance(m.content, str):
                system = m.content
            elif m.role == "user":
                if isinstance(m.content, str):
                    parts.append(m.content)
                else:
                    for c in m.content:
                        if c.get("type") == "text":
                            parts.append(c["text"])
                        elif c.get("type") == "image_url":
                            parts.append(load_image(c["image_url"]["url"]))
                        elif c.get("type") == "video_url":           # server.py:47-52, 214-221: `frames` (default 8) / `fps` (default 2) ride in the content
                            frames = c.get("frames", 8) if c.get("frames") is not None else 8
                            fps = c.get("fps", 2) if c.get("fps") is not None else 2
                            parts.append(Video(load_video_url_frames(c["video_url"]["url"], num_frames=int(frames), fps=float(fps))))
                        else:
                            raise NotImplementedError(f"Unsupported content type: {c.get('type')}")
            elif m.role == "assistant" and isinstance(m.content, str):
                parts.append(f"<|im_end|>\n<|im_start|>assistant\n{m.content}<|im_end|>\n<|im_start|>user\n")
        return parts, system

    model_lock = batcher.model_lock if isinstance(batcher, RequestBatcher) else threading.Lock()
    app.state.model_lock = model_lock

    def _solo(parts, n, system, temperature, top_p, streamer=None, **pen):
        """A request the batcher does not take: under the model lock — never beside the worker thread's batch, never beside another solo
        request."""
        with model_lock, torch.inference_mode():
            kw = {} if prompt_lookup_num_tokens is None else dict(prompt_lookup_num_tokens=prompt_lookup_num_tokens)
            kw.update(pen)                              # (non-neutral penalties only; generate_content then drops the speculation)
            top_k = kw.get("top_k", 50)                 # a request without the field samples with generate_content's default
            if spec_sample and kw and temperature and temperature > 0 and (1 <= top_k <= 64 or (any_top_k and top_k >= 0)):
                kw.update(spec_sample=True, top_k=top_k)
                if any_top_k and not 1 <= top_k <= 64:
                    kw.update(any_top_k=True)
            if spec_processed and prompt_lookup_num_tokens is not None:
                kw.update(spec_processed=True)
            return generate_content(model, tokenizer, parts, max_new_tokens=n, system=system, temperature=temperature, top_p=top_p, streamer=streamer, **kw)

    async def chat_completions(request):
        import asyncio
        try:
            under = request.model if bank is not None and request.model in bank else None     # vLLM's convention: `model` names a loaded adapter
            if under is None and request.model != model_name:
                raise ValueError(f"The endpoint is configured to use the model {model_name}, but the request model is {request.model}")
            parts, system = _prompt_of(request.messages)
            temperature = request.temperature if request.temperature is not None else 0.2
            top_p = request.top_p if request.top_p is not None else 0.9
            n = request.max_tokens or 512
            # non-neutral penalties only: a request that leaves them at 1 / 0 / 0 makes the calls it always made
            pen = _penalties_of(dict(repetition_penalty=request.repetition_penalty, presence_penalty=request.presence_penalty,
                                     frequency_penalty=request.frequency_penalty))
            # logprobs likewise: the two keywords travel with the penalties only for a request that asks
            n_top = _logprobs_of(getattr(request, "logprobs", None), getattr(request, "top_logprobs", None))
            if n_top is not None:
                if request.stream:
                    raise ValueError("`logprobs` is not served together with `stream`: true (entries on streamed pieces are not supported)")
                pen = dict(pen, logprobs=True, top_logprobs=n_top)
            # structured output likewise; refused with stream before anything runs
            pen = dict(pen, **check_structured_request({k: getattr(request, k, None) for k in STRUCTURED_FIELDS}, bool(request.stream)))
            # top_k likewise: it travels only for a sampled request that names one (-1, vLLM's "no filter", is HF's 0)
            top_k = getattr(request, "top_k", None)
            if top_k is not None:
                top_k = 0 if int(top_k) == -1 else int(top_k)
                if top_k < 0:
                    raise ValueError(f"`top_k` has to be a non-negative integer (0 or -1: no top-k filter), but is {request.top_k}")
                if temperature and temperature > 0:
                    pen = dict(pen, top_k=top_k)
            if under is not None:                                     # (the key travels only for a request under an adapter)
                pen = dict(pen, model=under)
            loop = asyncio.get_running_loop()
            if request.stream:
                # server.py:241-270: the reply leaves as it is generated.  The tokens reach a `TextStream` from whoever runs the request (the
                # continuous batcher's worker after every chunk of steps, else a thread of its own: the reference's Thread + TextIteratorStreamer)
                stream = TextStream(tokenizer, timeout=stream_timeout_s)
                if isinstance(batcher, ContinuousBatcher):
                    batcher.submit(parts, n, system, stream=stream, temperature=temperature, top_p=top_p, **pen)
                else:
                    def run():
                        try:
                            stream.finish(_solo(parts, n, system, temperature, top_p, streamer=stream, **pen))
                        except Exception as ex:                       # the consumer raises it
                            stream.fail(ex)
                    threading.Thread(target=run, daemon=True).start()
                first = await loop.run_in_executor(None, lambda: next(stream, None))      # a failure before any text is still a 500 body
                pieces = stream if first is None else itertools.chain([first], stream)
                return StreamingResponse(sse_chunks(pieces, request.model), media_type="text/event-stream")
            if isinstance(batcher, ContinuousBatcher):
                text = await loop.run_in_executor(None, batcher.submit(parts, n, system, temperature=temperature, top_p=top_p, **pen).result)
            elif batcher is not None and not temperature and not pen:
                text = await loop.run_in_executor(None, batcher.submit(parts, n, system).result)
            else:
                text = _solo(parts, n, system, temperature, top_p, **pen)
            choice: Dict[str, Any] = {"message": {"role": "assistant", "content": [{"type": "text", "text": str(text)}]}}
            if n_top is not None:
                choice["logprobs"] = {"content": list(getattr(text, "logprobs", None) or [])}
            return {"id": uuid.uuid4().hex, "object": "chat.completion", "created": time.time(), "model": request.model, "choices": [choice]}
        except Exception as e:                                       # server.py:292-297: errors come back as a 500 JSON body
            return JSONResponse(status_code=500, content={"error": str(e)})

    chat_completions.__annotations__["request"] = ChatCompletionRequest      # a real class, not a string (postponed annotations)
    app.post("/chat/completions")(chat_completions)
    return app
