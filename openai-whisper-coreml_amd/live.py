"""Live transcription of S audio streams that are still arriving (DESIGN.md "Live streams").

binding.Streams turns appended samples into log-mel frames on the device; LiveTranscriber decodes every due stream's
buffer [buf_first, avail) in ONE transcribe_mel call per step() and turns the successive, changing hypotheses into text
that is never taken back, by LocalAgreement-2 over token ids: what two consecutive hypotheses of a stream agree on
beyond the committed tokens is committed.

Per-stream state (StreamState; every transition below is a pure function that returns a new state):
    buf_first : absolute frame where the stream's buffer starts; always even (a timestamp token is 2 frames);
    committed : the generated tokens of the buffer that are final, timestamp tokens included, relative to buf_first;
    prev      : the last hypothesis beyond `committed`;
    context   : the committed TEXT tokens that have left the buffer (the prompt's previous text);
    stepped   : final_frames at the stream's last step (a stream is due min_step_frames later).
The GPU is touched in LiveTranscriber.push / step / finish alone."""
import collections

FRAMES_PER_TOKEN = 2        # a timestamp token is 0.02 s, a frame 0.01 s
FRAME_SECONDS = 0.01
MAX_WINDOW = 3000

StreamState = collections.namedtuple("StreamState", "buf_first committed prev context stepped")
Committed = collections.namedtuple("Committed", "tokens starts")   # newly committed ids and their absolute start times (s)


def new_state():
    return StreamState(0, (), (), (), 0)


def stream_prompt(context, sot_sequence, sot_prev, n_text_ctx):
    """[sot_prev, *context[-(n_text_ctx // 2 - 1):], *sot_sequence]; the sot_prev part is left out while context is empty."""
    seq = [int(t) for t in sot_sequence]
    if not context:
        return seq
    return [int(sot_prev)] + [int(t) for t in context[-(n_text_ctx // 2 - 1):]] + seq


def hypothesis_of(tokens, length, eot):
    """The generated tokens of a row without the stopping eot (and nothing behind it)."""
    out = []
    for t in list(tokens)[:int(length)]:
        if int(t) == int(eot):
            break
        out.append(int(t))
    return tuple(out)


def common_prefix(a, b):
    n = 0
    while n < len(a) and n < len(b) and a[n] == b[n]:
        n += 1
    return n


def token_starts(tokens, first, buf_first, timestamp_begin, opening=None):
    """Absolute start time (s) of tokens[first:] of a buffer that begins at frame buf_first: a text token starts at its
    segment's opening timestamp token -- the nearest timestamp token in front of it; buf_first's time when there is none
    -- and a timestamp token at its own time."""
    base = buf_first * FRAME_SECONDS
    cur = base if opening is None else opening
    out = []
    for i, t in enumerate(tokens):
        if t >= timestamp_begin:
            cur = base + (t - timestamp_begin) * FRAMES_PER_TOKEN * FRAME_SECONDS
        if i >= first:
            out.append(cur)
    return out


def agree(state, hyp, timestamp_begin):
    """LocalAgreement-2: hyp = the new hypothesis of the whole buffer (it begins with state.committed, which was given to
    the decode).  The longest common prefix of state.prev and hyp beyond committed is committed; prev becomes the rest.
    Returns (state, Committed)."""
    c = state.committed
    if tuple(hyp[:len(c)]) != tuple(c):
        raise ValueError("the hypothesis does not begin with the committed tokens it was given")
    tail = tuple(int(t) for t in hyp[len(c):])
    n = common_prefix(state.prev, tail)
    committed = c + tail[:n]
    new = Committed(list(tail[:n]), token_starts(committed, len(c), state.buf_first, timestamp_begin))
    return state._replace(committed=committed, prev=tail[n:]), new


def commit_all(state, timestamp_begin):
    """prev is committed whole (forced advance, finish).  Returns (state, Committed)."""
    c = state.committed + state.prev
    new = Committed(list(state.prev), token_starts(c, len(state.committed), state.buf_first, timestamp_begin))
    return state._replace(committed=c, prev=()), new


def last_pair(committed, timestamp_begin):
    """Index of <|e|> of the last adjacent pair of timestamp tokens <|e|><|s|> in committed, or None."""
    for i in range(len(committed) - 2, -1, -1):
        if committed[i] >= timestamp_begin and committed[i + 1] >= timestamp_begin:
            return i
    return None


def _cut(state, i, timestamp_begin):
    """committed[:i + 1] leave the buffer (committed[i] is a timestamp token <|e|>): their text ids go to context, buf_first
    advances by 2 (e - timestamp_begin) frames, every timestamp token left is lowered by e - timestamp_begin."""
    d = state.committed[i] - timestamp_begin

    def lower(toks):   # (a timestamp in front of the cut cannot follow it under the timestamp rules; it would read <|0.00|>)
        return tuple(max(t - d, timestamp_begin) if t >= timestamp_begin else t for t in toks)
    gone = tuple(t for t in state.committed[:i + 1] if t < timestamp_begin)
    return state._replace(buf_first=state.buf_first + FRAMES_PER_TOKEN * d, committed=lower(state.committed[i + 1:]),
                          prev=lower(state.prev), context=state.context + gone)


def _inside(state, i, avail, timestamp_begin):
    """a cut at committed[i] leaves a buffer of at least one frame (a timestamp may lie behind the audio that has arrived:
    the decode pads a short window with silence)"""
    return state.buf_first + FRAMES_PER_TOKEN * (state.committed[i] - timestamp_begin) < avail


def trim(state, avail, trim_frames, timestamp_begin):
    """If the buffer holds more than trim_frames frames and committed has an adjacent timestamp pair <|e|><|s|>, the tokens
    up to and including the last pair's <|e|> leave the buffer.  Returns (state, trimmed?)."""
    i = last_pair(state.committed, timestamp_begin)
    if avail - state.buf_first <= trim_frames or i is None or not _inside(state, i, avail, timestamp_begin):
        return state, False
    return _cut(state, i, timestamp_begin), True


def force_advance(state, avail, trim_frames, timestamp_begin):
    """The buffer would outgrow a window and nothing can be trimmed: prev is committed whole and the buffer is cut at the
    last timestamp token.  Without tokens -- or when that cut would not move the buffer (the token is <|0.00|>) -- the
    buffer moves to the even frame at or below avail - trim_frames: committed text goes to context and prev is cleared.
    Returns (state, Committed)."""
    state, new = commit_all(state, timestamp_begin)
    ts = [i for i, t in enumerate(state.committed) if t >= timestamp_begin]
    if ts and state.committed[ts[-1]] > timestamp_begin and _inside(state, ts[-1], avail, timestamp_begin):
        return _cut(state, ts[-1], timestamp_begin), new
    first = max(state.buf_first, (avail - trim_frames) // 2 * 2)
    gone = tuple(t for t in state.committed if t < timestamp_begin)
    return state._replace(buf_first=first, committed=(), prev=(), context=state.context + gone), new


def after_hypothesis(state, hyp, avail, final, *, timestamp_begin, trim_frames=1500, min_step_frames=100):
    """One step of a stream as a pure function: agreement, trim, and the forced advance when the buffer would exceed a
    window (3000 frames) at the next step and nothing could be trimmed.  Returns (state, Committed)."""
    state, new = agree(state, hyp, timestamp_begin)
    state, cut = trim(state, avail, trim_frames, timestamp_begin)
    if not cut and avail - state.buf_first + min_step_frames > MAX_WINDOW:
        state, more = force_advance(state, avail, trim_frames, timestamp_begin)
        new = Committed(new.tokens + more.tokens, new.starts + more.starts)
    return state._replace(stepped=final), new


def before_decode(state, avail, trim_frames, timestamp_begin):
    """A buffer that has outgrown a window before it could be decoded (more audio arrived between two steps than a step
    allows for) is advanced first.  Returns (state, Committed)."""
    new = Committed([], [])
    while avail - state.buf_first > MAX_WINDOW:
        state, more = force_advance(state, avail, trim_frames, timestamp_begin)
        new = Committed(new.tokens + more.tokens, new.starts + more.starts)
    return state, new


def is_due(state, final, min_step_frames):
    return final - state.stepped >= min_step_frames


class LiveTranscriber:
    """S live streams on one model context.  push() appends audio (16 kHz), step() decodes every due stream once and returns
    {stream: (Committed, tail)} -- the newly committed tokens with their absolute start times, and the current unconfirmed
    tail --, finish(s) decodes once more, commits the whole hypothesis and resets the stream.

    sot, language, task, eot, timestamp_begin, sot_prev, no_speech_token: the token ids binding.transcribe_long takes.
    Out of scope, and refused: rates other than 16 kHz (the resampler keeps no state between calls), best-of, beam search and
    temperature fallback."""

    def __init__(self, ctx, S, *, sot, language, task, eot, timestamp_begin, sot_prev, no_speech_token=-1, sample_rate=16000,
                 min_step_frames=100, trim_frames=1500, capacity_frames=3003, max_initial_timestamp=1.0, best_of=None, beam_size=None,
                 temperatures=None):
        from . import binding
        if int(sample_rate) != 16000:
            raise ValueError("live streams take 16 kHz audio: the resampler keeps no state between calls")
        if best_of is not None or beam_size is not None:
            raise ValueError("live streams decode one arg-max sample per stream: best_of and beam_size are not served")
        if temperatures is not None and tuple(temperatures) not in ((), (0.0,), (0,)):
            raise ValueError("live streams decode at temperature 0: temperature fallback is not served")
        if ctx.dims is None:
            raise ValueError("LiveTranscriber needs a model context")
        if not 1 <= int(min_step_frames) <= int(trim_frames) <= MAX_WINDOW - int(min_step_frames):
            raise ValueError("need 1 <= min_step_frames <= trim_frames <= 3000 - min_step_frames")
        self.b, self.ctx, self.S = binding, ctx, int(S)
        self.sot_sequence = [int(sot), int(language), int(task)]
        self.eot, self.timestamp_begin, self.sot_prev = int(eot), int(timestamp_begin), int(sot_prev)
        self.no_speech_token = int(no_speech_token)
        self.min_step_frames, self.trim_frames = int(min_step_frames), int(trim_frames)
        self.max_initial = int(round(float(max_initial_timestamp) / (FRAMES_PER_TOKEN * FRAME_SECONDS)))
        self.n_ctx = int(ctx.dims["n_text_ctx"])
        self.max_new = min(self.n_ctx // 2, self.n_ctx - (self.n_ctx // 2 + 3))
        self.streams = binding.Streams(ctx, self.S, n_mels=int(ctx.dims["n_mels"]), capacity_frames=capacity_frames)
        self.state = [new_state() for _ in range(self.S)]
        self.last = {}   # stream -> (first frame, frames, prompt, given, hypothesis) of its last decode

    def close(self):
        self.streams.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def push(self, pieces):
        """One array of new samples per stream (None: nothing)."""
        self.streams.push(pieces)

    def _decode(self, rows):
        """ONE window call and ONE transcribe_mel call for the streams `rows`; their hypotheses."""
        _, _, avail, _ = self.streams.frames()
        wins = [(s, self.state[s].buf_first, int(avail[s]) - self.state[s].buf_first) for s in rows]
        prompts = [stream_prompt(self.state[s].context, self.sot_sequence, self.sot_prev, self.n_ctx) for s in rows]
        given = [list(self.state[s].committed) for s in rows]
        d_mel, base, n = self.streams.window(wins, device=True)
        try:
            self.ctx.set_timestamp_rules(True, self.timestamp_begin, self.eot, self.max_initial)
            r = self.ctx.transcribe_mel(d_mel, base, n, 0, n, prompts, self.max_new, eot=self.eot,
                                        no_speech_token=self.no_speech_token, mem=self.b.WM_MEM_DEVICE, sot_tail=3,
                                        given=given if any(given) else None)
        finally:
            self.ctx.dev_free(d_mel)
        hyps = [hypothesis_of(r.tokens[i], r.lens[i], self.eot) for i in range(len(rows))]
        for i, s in enumerate(rows):
            self.last[s] = (wins[i][1], wins[i][2], prompts[i], given[i], hyps[i])
        return hyps

    def step(self):
        _, final, avail, _ = self.streams.frames()
        due = [s for s in range(self.S) if is_due(self.state[s], int(final[s]), self.min_step_frames)]
        if not due:
            return {}
        early = {}
        for s in due:
            self.state[s], early[s] = before_decode(self.state[s], int(avail[s]), self.trim_frames, self.timestamp_begin)
        out = {}
        for s, hyp in zip(due, self._decode(due)):
            self.state[s], new = after_hypothesis(self.state[s], hyp, int(avail[s]), int(final[s]),
                                                  timestamp_begin=self.timestamp_begin, trim_frames=self.trim_frames,
                                                  min_step_frames=self.min_step_frames)
            new = Committed(early[s].tokens + new.tokens, early[s].starts + new.starts)
            out[s] = (new, list(self.state[s].prev))
        return out

    def finish(self, s):
        """Stream s has ended: one more decode, the whole hypothesis is committed, the stream is reset.  Returns Committed."""
        s = int(s)
        _, _, avail, _ = self.streams.frames()
        new = Committed([], [])
        if int(avail[s]) > 0:
            self.state[s], new = before_decode(self.state[s], int(avail[s]), self.trim_frames, self.timestamp_begin)
            hyp = self._decode([s])[0]
            st, a = agree(self.state[s], hyp, self.timestamp_begin)
            st, b = commit_all(st, self.timestamp_begin)
            new = Committed(new.tokens + a.tokens + b.tokens, new.starts + a.starts + b.starts)
        self.streams.reset(s)
        self.state[s] = new_state()
        self.last.pop(s, None)
        return new
