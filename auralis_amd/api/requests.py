"""TTSRequest — same fields, defaults and meaning as the reference dataclass
(src/auralis/common/definitions/requests.py:134-277).  Fields the reference carries but never consumes on the
synthesis path (do_sample, length_penalty, sound_norm_refs, load_sample_rate) are kept for
drop-in compatibility.  `seed` is new surface (per-request noise stream; the reference has none); so are `priority`, `speed`,
`output_sample_rate` and `output_encoding`."""
from __future__ import annotations

import copy as _copy
import math
import uuid
from dataclasses import dataclass, field
from typing import AsyncGenerator, Callable, List, Optional, Union

from .lang import get_language, validate_language

# the rates the engine delivers (aur_seq_desc.sample_rate; include/auralis_amd.h)
OUTPUT_SAMPLE_RATES = (8000, 16000, 22050, 24000, 32000, 44100, 48000)
# what the engine encodes behind the vocoder (aur_seq_desc.encoding)
OUTPUT_ENCODINGS = (None, "flac")


@dataclass
class AudioPreprocessingConfig:
    """Options of the optional reference-audio enhancer (requests.py:171, enhancer.py:34-153): carried, unused here."""
    sample_rate: int = 22050
    normalize: bool = True
    trim_silence: bool = True
    remove_noise: bool = True
    enhance_speech: bool = True


@dataclass
class TTSRequest:
    text: Union[AsyncGenerator[str, None], str, List[str]]
    speaker_files: Union[str, List[str], bytes, List[bytes]]
    context_partial_function: Optional[Callable] = None
    start_time: Optional[float] = None
    enhance_speech: bool = False
    audio_config: AudioPreprocessingConfig = field(default_factory=AudioPreprocessingConfig)
    language: str = "auto"
    request_id: str = field(default_factory=lambda: uuid.uuid4().hex)
    load_sample_rate: int = 22050
    sound_norm_refs: bool = False
    # voice conditioning
    max_ref_length: int = 60
    gpt_cond_len: int = 30
    gpt_cond_chunk_len: int = 4
    # generation
    stream: bool = False
    temperature: float = 0.75
    top_p: float = 0.85
    top_k: int = 50
    repetition_penalty: float = 5.0
    length_penalty: float = 1.0
    do_sample: bool = True
    seed: Optional[int] = None
    # new surface, like `seed`: > 0 marks the request latency-critical -- its FIRST chunk is what a listener waits for -- and is
    # handed to the engine as aur_seq_desc.priority (the reference has no such knob: tests/integration/stream_ttfb.py only measures)
    priority: int = 0
    # new surface, like `seed` and `priority`: the speaking rate, 0.5 <= speed <= 2.0, handed to the engine as aur_seq_desc.speed for
    # every chunk of the request -- the GPT latents are stretched along time by 1 / speed ahead of the vocoder (the XTTS
    # inference(speed=) rule), so pitch and loudness stay and nothing runs on the finished waveform (the reference's only speed
    # control is TTSOutput.change_speed, a phase vocoder over the audio)
    speed: float = 1.0
    # new surface, like `speed`: the sample rate of the audio the request yields, one of OUTPUT_SAMPLE_RATES, handed to the engine as
    # aur_seq_desc.sample_rate for every chunk -- the GPU resamples behind the vocoder (torchaudio's windowed sinc, the rule of the
    # reference's TTSOutput.resample) and stores the result where the 24 kHz waveform would have gone; nothing runs on the host
    output_sample_rate: int = 24000
    # new surface, like `output_sample_rate`: None, or "flac" -- every chunk is also encoded to a 16-bit FLAC stream on the GPU behind
    # the vocoder (aur_seq_desc.encoding) and its TTSOutput carries the bytes (`encoded`), which to_bytes("flac") then returns instead of
    # running the host writer.  The float audio is delivered as ever
    output_encoding: Optional[str] = None

    def __post_init__(self):
        if self.output_encoding not in OUTPUT_ENCODINGS:
            raise ValueError(f"output_encoding must be one of {OUTPUT_ENCODINGS}, got {self.output_encoding!r}")
        if isinstance(self.output_sample_rate, bool) or not isinstance(self.output_sample_rate, int) \
                or self.output_sample_rate not in OUTPUT_SAMPLE_RATES:
            raise ValueError(f"output_sample_rate must be one of {OUTPUT_SAMPLE_RATES}, got {self.output_sample_rate!r}")
        try:
            ok = math.isfinite(self.speed) and 0.5 <= float(self.speed) <= 2.0
        except TypeError:
            ok = False
        if not ok:
            raise ValueError(f"speed must be a finite number in [0.5, 2.0], got {self.speed!r}")
        if self.language == "auto" and isinstance(self.text, str) and len(self.text) > 0:
            self.language = get_language(self.text)
        validate_language(self.language)

    def infer_language(self) -> None:
        """Detect the language of `text` when it is "auto" (the reference's requests.py method of the same name)."""
        if self.language == "auto" and isinstance(self.text, str) and len(self.text) > 0:
            self.language = get_language(self.text)

    def copy(self) -> "TTSRequest":
        return _copy.copy(self)
