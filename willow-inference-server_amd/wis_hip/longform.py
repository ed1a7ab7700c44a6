"""Long-form transcription: openai-whisper's `transcribe()` seek loop over one whole-recording log-mel (audio.LongMel), restated.

The decode step is injected, so the rule runs without a model (tests/test_longform_cpu.py):

    decode(window, prompt, temperature, n) -> ([(tokens, score), ...], no_speech_prob)

`window` is what `long_mel.window(seek)` gave (a device address for audio.LongMel: valid until the next window is asked for), `prompt` the
assembled decoder prompt, `temperature` / `n` as whisper.decode_with_fallback hands them (0: the search, n = 1; else n samples), `score` the
engine's (cumulative log-probability over the token count).  The prompt always asks for timestamps: the loop needs them to know where a window's
text ends, whether or not the caller returns segments.

The rule, per window at `seek` (frames of 10 ms) while seek < long_mel.frames, with segment_size = min(3000, frames - seek) and
time_offset = 0.01 seek:

  * decode under whisper.decode_with_fallback (no temperatures: one search);
  * no_speech_threshold set and no_speech_prob above it: the window is skipped (seek += segment_size, no segment) - unless logprob_threshold is
    set and the kept decode's average log-probability is above it;
  * consecutive timestamp pairs split the tokens into segments, start / end = time_offset + 0.02 (first / last timestamp - <|0.00|>); when the
    last two tokens are (text, timestamp) that single timestamp closes a final slice and seek += segment_size, otherwise seek advances to the last
    closed timestamp, 2 (timestamp - <|0.00|>) frames, and what follows it is decoded again by the next window;
  * no pairs: one segment from time_offset to the last timestamp seen if that is not <|0.00|>, else to the window's end; seek += segment_size;
  * the next window's prompt is initial_prompt_ids + the text tokens of every kept segment since the last reset, cut from the left by
    whisper.assemble_prompt; a reset happens when condition_on_previous_text is off or the kept decode's temperature is above 0.5.

Three deviations from openai-whisper in this loop: the conditioning text carries text tokens only (assemble_prompt's contract; the original keeps
the timestamp tokens); an advance of zero frames (a pair that closes at <|0.00|>) is replaced by segment_size, where the original loop would
stall; and segment times are held inside the window's content: the decoder may close a segment of a short last window at a timestamp behind the
recording's end, which the original reports as it is.  (A fourth lives in whisper.do_whisper: words are held inside their segments.)
"""
from .whisper import assemble_prompt, decode_with_fallback

N_FRAMES = 3000                # frames of one window
FRAME_S = 0.01                 # one mel frame
TIME_PRECISION = 0.02          # one timestamp token
RESET_TEMPERATURE = 0.5


def split_window(tokens, timestamp_begin, time_offset, segment_size):
    """One window's tokens (no <|endoftext|>) -> (segments [{start, end, tokens}], advance in frames before the zero guard)."""
    toks = [int(t) for t in tokens]
    is_ts = [t >= timestamp_begin for t in toks]
    single_timestamp_ending = is_ts[-2:] == [False, True]
    slices = [i + 1 for i in range(len(toks) - 1) if is_ts[i] and is_ts[i + 1]]
    segments = []

    content = segment_size * FRAME_S      # a timestamp behind the window's content (a short last window) is held at the recording's end

    def seg(start, end, piece):
        segments.append({"start": round(time_offset + min(start, content), 2), "end": round(time_offset + min(end, content), 2), "tokens": list(piece)})
    if slices:
        if single_timestamp_ending:
            slices.append(len(toks))
        last = 0
        for cur in slices:
            piece = toks[last:cur]
            seg((piece[0] - timestamp_begin) * TIME_PRECISION, (piece[-1] - timestamp_begin) * TIME_PRECISION, piece)
            last = cur
        if single_timestamp_ending:
            return segments, segment_size
        return segments, 2 * (toks[last - 1] - timestamp_begin)
    stamps = [t for t in toks if t >= timestamp_begin]
    duration = segment_size * FRAME_S
    if stamps and stamps[-1] != timestamp_begin:
        duration = (stamps[-1] - timestamp_begin) * TIME_PRECISION
    seg(0.0, duration, toks)
    return segments, segment_size


def transcribe(long_mel, decode, *, start, special, initial_prompt_ids=(), n_text_ctx=448, temperatures=(), best_of=5, compression_ratio_threshold=None,
               logprob_threshold=None, no_speech_threshold=0.6, condition_on_previous_text=True, text_of=None, on_window=None, encode=None):
    """The loop of the module text.  long_mel: `.frames` and `.window(seek)`; start: the start sequence WITHOUT <|notimestamps|>; special: the
    model's SpecialTokens (timestamp_begin, eot, startofprev); text_of: tokens -> text for the fallback's compression ratio (None: off);
    on_window(window, seek, segment_size, segments): called for every kept window while `window` is still valid (word alignment).
    encode(window, seek): called once per window; what it returns (the window's encoder output, say) is what `decode` and `on_window` get as
    `window` - every decode of the fallback and the alignment then read one encoder pass.
    -> dict(segments=[{start, end, tokens, ...}], windows=[one dict per decoded window: seek, segment_size, prompt, tokens, temperature,
    avg_logprob, no_speech_prob, skipped, advance], fallback=the last kept decode's decode_with_fallback result)"""
    tb, eot = special.timestamp_begin, special.eot
    temps = tuple(temperatures) or (0.0,)
    frames = int(long_mel.frames)
    history, segments, windows, fallback = [], [], [], None
    seek = 0
    while seek < frames:
        segment_size = min(N_FRAMES, frames - seek)
        time_offset = round(seek * FRAME_S, 2)
        prompt = assemble_prompt(start, special, list(initial_prompt_ids) + history, (), n_text_ctx)
        window = long_mel.window(seek)
        if encode is not None:
            window = encode(window, seek)
        nsp = [0.0]

        def step(t, n):
            cands, nsp[0] = decode(window, prompt, t, n)
            return [([int(x) for x in toks if int(x) != eot], score) for toks, score in cands]
        fb = decode_with_fallback(step, temps, best_of, compression_ratio_threshold, logprob_threshold, text_of)
        tokens = fb["tokens"]
        rec = dict(seek=seek, segment_size=segment_size, prompt=prompt, tokens=tokens, temperature=fb["temperature"], avg_logprob=fb["avg_logprob"],
                   no_speech_prob=float(nsp[0]), skipped=False)
        windows.append(rec)
        if no_speech_threshold is not None and nsp[0] > no_speech_threshold and not (logprob_threshold is not None and fb["avg_logprob"] > logprob_threshold):
            rec["skipped"], rec["advance"] = True, segment_size
            seek += segment_size
            continue
        segs, advance = split_window(tokens, tb, time_offset, segment_size)
        if advance <= 0:
            advance = segment_size
        rec["advance"] = advance
        if on_window is not None:
            on_window(window, seek, segment_size, segs)
        segments.extend(segs)
        fallback = fb
        if not condition_on_previous_text or fb["temperature"] > RESET_TEMPERATURE:
            history = []
        else:
            history.extend(t for sg in segs for t in sg["tokens"] if t < eot)
            history = history[-n_text_ctx:]      # (more than the prompt can ever hold)
        seek += advance
    return dict(segments=segments, windows=windows, fallback=fallback)
