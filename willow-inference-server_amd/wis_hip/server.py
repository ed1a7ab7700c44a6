"""Thin re-host of the reference's REST ASR endpoints over the HIP path:

    GET  /api/ping      (main.py:1129-1137)
    POST /api/asr       multipart upload `audio_file`             (main.py:1168-1234)
    POST /api/willow    raw body + x-audio-* headers              (main.py:1237-1377)

Same query parameters, same JSON fields, same 400 behaviour (`{"error": "Invalid force_language"}`, `{"error": "Invalid
audio"}`).  Differences, all deliberate:
  * inference runs OFF the event loop (a thread pool calls `do_whisper`; ctypes releases the GIL), so concurrent requests
    reach the model together and the micro-batcher (wis_hip/batching.py) turns them into device batches - the reference blocks
    its single worker inside `do_whisper` (main.py:1205, 1338);
  * audio containers: WAV, FLAC and raw PCM are decoded natively (csrc/audio_io.c); other codecs need PyAV, which the
    reference uses (`audio_to_wav`, main.py:108-120) and this image does not have -> HTTP 400 "Invalid audio";
  * speaker verification (`voice_auth=true`, main.py:1324-1360) is served when `support_sv` is set (wis_hip/sv.py, the WavLM x-vector
    embedder in csrc/sv.hip): it runs on the thread pool before Whisper, answers 406 "Unauthorized voice" when no enrolled speaker
    reaches `sv_threshold`, else adds `voice_auth` and `speaker_status` to the (stats) JSON.  Without `support_sv` (the default) a
    `voice_auth` request is answered HTTP 400, where the reference would fail inside `do_sv`.
WebRTC (`/api/rtc/asr`), TTS, nginx auth and the static sites are not re-hosted (out of scope).

    python -m wis_hip.server --host 0.0.0.0 --port 19000        (or: uvicorn --factory wis_hip.server:create_app ...)
"""
import asyncio
import io
import logging
import math
import os
import wave
from concurrent.futures import ThreadPoolExecutor
from contextlib import asynccontextmanager
from email.parser import BytesParser
from email.policy import HTTP

from fastapi import FastAPI, Request
from fastapi.middleware.cors import CORSMiddleware
from fastapi.responses import JSONResponse, PlainTextResponse

from .settings import get_api_settings
from .whisper import InvalidAudio, WhisperModels, check_model_language, do_whisper

logger = logging.getLogger("infer")


def write_stream_wav(data, rate, bits, ch):
    """Raw PCM from a Willow device -> in-memory WAV (main.py:98-105)."""
    f = io.BytesIO()
    w = wave.open(f, "wb")
    w.setparams((ch, bits // 8, rate, 0, "NONE", "NONE"))
    w.writeframesraw(bytes(data))
    w.close()
    f.seek(0)
    return f


def _multipart_boundary(content_type):
    for piece in (content_type or "").split(";")[1:]:
        k, _, v = piece.strip().partition("=")
        if k.strip().lower() == "boundary":
            return v.strip().strip('"').encode("latin-1")
    return None


def parse_multipart(body, content_type, field="audio_file"):
    """The one multipart field /api/asr needs (python-multipart is not installed, so FastAPI's UploadFile is unavailable).
    Parts are located with bytes.find on the boundary and only the part HEADERS go through the e-mail header parser: the payload
    (the uploaded audio, tens of kilobytes to megabytes) is sliced, never scanned line by line - the generic MIME parser spent
    2.6 ms of GIL-held time on the 67 KB reference clip, the largest per-request cost of the host path (tools/host_ceiling.py)."""
    if "multipart/form-data" not in (content_type or ""):
        raise ValueError("expected multipart/form-data")
    boundary = _multipart_boundary(content_type)
    if not boundary:
        raise ValueError("multipart boundary missing")
    body = bytes(body) if not isinstance(body, bytes) else body
    delim = b"--" + boundary
    pos = body.find(delim)
    while pos >= 0:
        start = pos + len(delim)
        if body[start:start + 2] == b"--":           # closing delimiter
            break
        eol = body.find(b"\r\n", start)
        if eol < 0:
            break
        head_end = body.find(b"\r\n\r\n", eol)
        if head_end < 0:
            break
        nxt = body.find(b"\r\n" + delim, head_end + 4)
        if nxt < 0:
            raise ValueError("multipart body is not terminated")
        headers = BytesParser(policy=HTTP).parsebytes(body[eol + 2:head_end] + b"\r\n\r\n", headersonly=True)
        if headers.get_param("name", header="content-disposition") == field:
            payload = body[head_end + 4:nxt]
            cte = (headers.get("content-transfer-encoding") or "").strip().lower()
            if cte == "base64":
                import base64
                payload = base64.b64decode(payload)
            elif cte == "quoted-printable":
                import quopri
                payload = quopri.decodestring(payload)
            return payload
        pos = nxt + 2
    raise ValueError(f"multipart field {field!r} missing")


class BadRequest(ValueError):
    """A request parameter the engine cannot serve -> HTTP 400 with the message."""


def _json_matches(matches):
    """do_whisper's `matches` for a JSON body: a logmass / in_grammar that is no finite number (-inf: the list allowed nothing of the model's
    probability; NaN: a step the search never scored) is sent as null."""
    return [{k: (None if isinstance(v, float) and not math.isfinite(v) else v) for k, v in m.items()} for m in matches]


def _as_bool(v, default):
    if v is None:
        return default
    return str(v).strip().lower() in ("1", "true", "yes", "on")


def create_app(models=None, settings=None, max_workers=None, sv=None):
    """sv: the speaker verifier (an object with `embed(pcm)`, e.g. wis_hip.sv.SpeakerVerifier); None = created on first use from
    `sv_model_path` when `support_sv` is set"""
    s = settings or (models.settings if models is not None else get_api_settings())
    if getattr(s, "long_form", "chunk") not in ("chunk", "seek"):      # (a bad setting fails the start, not every request)
        raise ValueError(f"setting long_form {s.long_form!r}: seek or chunk")
    if getattr(s, "phrases_file", ""):      # (an unreadable phrase list fails the start too)
        from .whisper import load_phrases_file
        if not load_phrases_file(s.phrases_file):
            raise ValueError(f"setting phrases_file {s.phrases_file!r}: the file holds no phrase")
    if getattr(s, "hotwords_file", ""):      # (and an unreadable or empty hotword list; a boost of 0 beside it is "off", anything else must be a boost)
        from .whisper import load_hotwords_file
        if not load_hotwords_file(s.hotwords_file):
            raise ValueError(f"setting hotwords_file {s.hotwords_file!r}: the file holds no entry")
    hb = getattr(s, "hotword_boost", 0.0)
    if not (isinstance(hb, (int, float)) and math.isfinite(hb) and hb >= 0):
        raise ValueError(f"setting hotword_boost {hb!r}: a finite number > 0, or 0 for off")
    if getattr(s, "phrases_file", "") and getattr(s, "hotwords_file", "") and hb > 0:      # (every request would be constrained: the hotword list could never apply)
        raise ValueError("settings phrases_file and hotwords_file / hotword_boost: a constrained search has nothing left to bias - set one of them")
    state = {"models": models, "sv": sv}
    sv_lock = __import__("threading").Lock()
    # enough threads that a full device batch per GPU replica can be waiting in the micro-batcher at once
    pool = ThreadPoolExecutor(max_workers=max_workers or 8 * max(1, s.max_batch), thread_name_prefix="wis-req")

    def get_models():
        if state["models"] is None:
            state["models"] = WhisperModels(s)
        return state["models"]

    @asynccontextmanager
    async def lifespan(_app):       # main.py:1097-1101: load, then warm on the reference clip when one is configured
        if os.environ.get("WIS_PRELOAD", "0") == "1":
            m = get_models()
            m.preload()
            clip = os.environ.get("WIS_WARM_CLIP")
            if clip and os.path.exists(clip):
                m.warm(clip)
        yield
        pool.shutdown(wait=False, cancel_futures=True)

    app = FastAPI(title=s.name, description=s.description, version=s.version, openapi_url="/api/openapi.json", docs_url="/api/docs",
                  redoc_url="/api/redoc", lifespan=lifespan)
    if s.cors_allowed_origins:
        app.add_middleware(CORSMiddleware, allow_origins=s.cors_allowed_origins, allow_credentials=True, allow_methods=["*"], allow_headers=["*"])

    def params(request):
        q = request.query_params
        model = q.get("model", s.whisper_model_default)
        beam = q.get("beam_size")
        try:
            beam = int(beam) if beam not in (None, "") else s.beam_size
        except ValueError:
            raise BadRequest(f"Invalid beam_size {beam!r}")
        # the engine's beam ceiling is a property of the request, not a server fault (the reference accepts any int, main.py:1180)
        if not 1 <= beam <= s.max_beam:
            raise BadRequest(f"beam_size {beam} outside 1..{s.max_beam}")
        # CTranslate2's two options against looping hypotheses: absent = the settings' values; unparsable or out of range = 400
        rp, ng = q.get("repetition_penalty"), q.get("no_repeat_ngram_size")
        try:
            rp = float(rp) if rp not in (None, "") else None
            ng = int(ng) if ng not in (None, "") else None
        except ValueError:
            raise BadRequest(f"Invalid repetition_penalty {rp!r} / no_repeat_ngram_size {ng!r}")
        if rp is not None and not (0 < rp < float("inf")):
            raise BadRequest(f"repetition_penalty {rp} must be a finite number > 0")
        if ng is not None and ng < 0:
            raise BadRequest(f"no_repeat_ngram_size {ng} must be >= 0")
        # openai-whisper's temperature fallback: temperatures=0,0.2,0.4 and best_of= per request (absent: the settings' values); a bad value = 400
        temps, best_of = q.get("temperatures"), q.get("best_of")
        if temps in (None, ""):
            temps = None
        if best_of in (None, ""):
            best_of = None
        if temps is not None or best_of is not None:
            from .whisper import parse_temperatures
            try:
                t_, n_ = parse_temperatures(temps if temps is not None else (), best_of if best_of is not None else 1)
            except ValueError as e:
                raise BadRequest(f"Invalid temperatures / best_of: {e}")
            temps, best_of = (t_ if temps is not None else None), (n_ if best_of is not None else None)
            if best_of is not None and best_of > s.max_beam:
                raise BadRequest(f"best_of {best_of} outside 1..{s.max_beam}")
        # openai-whisper's initial_prompt= / prefix=: text, or "ids:1,2,3" for token ids; absent or empty = the settings' values; unparsable = 400
        prompts = {}
        for name in ("initial_prompt", "prefix"):
            v = q.get(name)
            if v in (None, ""):
                prompts[name] = None
            elif len(v) > 4096:
                raise BadRequest(f"{name}: {len(v)} characters (at most 4096)")
            elif v.startswith("ids:"):
                try:
                    prompts[name] = [int(t) for t in v[4:].split(",") if t.strip() != ""]
                except ValueError:
                    raise BadRequest(f"Invalid {name} {v!r}: ids:<comma-separated token ids>")
                if any(t < 0 for t in prompts[name]):
                    raise BadRequest(f"Invalid {name} {v!r}: token ids are >= 0")
            else:
                prompts[name] = v
        # phrase-constrained decoding: phrases=a|b|c (text; an entry "ids:1,2,3" is token ids) and phrase_nbest=n; absent or empty = the setting's list
        # (phrases_file) and 1; unparsable = 400
        def entry_list(name):
            raw = q.get(name)
            if raw in (None, ""):
                return None
            if len(raw) > 65536:
                raise BadRequest(f"{name}: {len(raw)} characters (at most 65536)")
            entries = []
            for v in raw.split("|"):
                if v.strip() == "":
                    raise BadRequest(f"Invalid {name} {raw!r}: an empty entry")
                if v.startswith("ids:"):
                    try:
                        v = [int(t) for t in v[4:].split(",") if t.strip() != ""]
                    except ValueError:
                        raise BadRequest(f"Invalid {name} entry {v!r}: ids:<comma-separated token ids>")
                    if not v or any(t < 0 for t in v):
                        raise BadRequest(f"Invalid {name}: an ids: entry holds token ids >= 0, at least one")
                entries.append(v)
            return entries
        phrases, nbest = entry_list("phrases"), q.get("phrase_nbest")
        # hotword boosting: hotwords=a|b|ids:400,401 (entries as in phrases=) and hotword_boost=2.5 (finite, > 0); absent or empty = the settings'
        # list (hotwords_file) and boost (hotword_boost, 0 = off); a list without any boost, or together with phrases, = 400 (do_whisper's ValueError)
        hotwords, hboost = entry_list("hotwords"), q.get("hotword_boost")
        try:
            hboost = float(hboost) if hboost not in (None, "") else None
        except ValueError:
            raise BadRequest(f"Invalid hotword_boost {hboost!r}")
        if hboost is not None and not (0 < hboost < float("inf")):      # (a NaN fails both comparisons)
            raise BadRequest(f"hotword_boost {hboost!r} must be a finite number > 0")
        try:
            nbest = int(nbest) if nbest not in (None, "") else None
        except ValueError:
            raise BadRequest(f"Invalid phrase_nbest {nbest!r}")
        if nbest is not None and not 1 <= nbest <= s.max_beam:
            raise BadRequest(f"phrase_nbest {nbest} outside 1..{s.max_beam}")
        # the out-of-grammar signal: phrase_mass=true | false, phrase_threshold=0.2 (a number in [0, 1]), phrase_fallback=true | false; absent or empty =
        # the settings' values; anything else = 400
        pm = {}
        for name in ("phrase_mass", "phrase_fallback"):
            v = q.get(name)
            if v in (None, ""):
                pm[name] = None
            elif str(v).strip().lower() in ("1", "true", "yes", "on"):
                pm[name] = True
            elif str(v).strip().lower() in ("0", "false", "no", "off"):
                pm[name] = False
            else:
                raise BadRequest(f"Invalid {name} {v!r}: true or false")
        pthr = q.get("phrase_threshold")
        try:
            pthr = float(pthr) if pthr not in (None, "") else None
        except ValueError:
            raise BadRequest(f"Invalid phrase_threshold {pthr!r}")
        if pthr is not None and not 0.0 <= pthr <= 1.0:      # (a NaN fails both comparisons)
            raise BadRequest(f"phrase_threshold {pthr!r} outside [0, 1]")
        pm["phrase_threshold"] = pthr
        # recordings over 30 s: long_form=seek | chunk, condition_on_previous_text=, no_speech_threshold= (absent: the settings' values); a bad value = 400
        lf = q.get("long_form") or None
        if lf is not None and lf not in ("seek", "chunk"):
            raise BadRequest(f"Invalid long_form {lf!r}: seek or chunk")
        cond = q.get("condition_on_previous_text")
        if cond in (None, ""):
            cond = None
        elif cond.strip().lower() in ("1", "true", "yes", "on", "0", "false", "no", "off"):
            cond = _as_bool(cond, True)
        else:
            raise BadRequest(f"Invalid condition_on_previous_text {cond!r}: true or false")
        nst = q.get("no_speech_threshold")
        try:
            nst = float(nst) if nst not in (None, "") else None
        except ValueError:
            raise BadRequest(f"Invalid no_speech_threshold {nst!r}")
        if nst is not None and nst != nst:
            raise BadRequest("Invalid no_speech_threshold: not a number")
        return dict(model=model, beam_size=beam, repetition_penalty=rp, **prompts, no_repeat_ngram_size=ng, temperatures=temps, best_of=best_of,
                    long_form=lf, condition_on_previous_text=cond, no_speech_threshold=nst, phrases=phrases, phrase_nbest=nbest, **pm,
                    hotwords=hotwords, hotword_boost=hboost,
                    detect_language=_as_bool(q.get("detect_language"), s.detect_language), force_language=q.get("force_language") or None,
                    translate=_as_bool(q.get("translate"), False), timestamps=_as_bool(q.get("timestamps"), False),
                    word_timestamps=_as_bool(q.get("word_timestamps"), False))

    async def run_whisper(audio_file, p):
        loop = asyncio.get_running_loop()
        kw = {"timestamps": True} if p["timestamps"] else {}      # (segment times; audio over 30 s is a 400 unless long_form=seek)
        if p["word_timestamps"]:                                  # (word times imply segment times; no vocabulary is a 400, and so is audio over 30 s without long_form=seek)
            kw = {"word_timestamps": True}
        kw.update({k: p[k] for k in ("repetition_penalty", "no_repeat_ngram_size", "temperatures", "best_of", "initial_prompt", "prefix", "long_form",
                                         "condition_on_previous_text", "no_speech_threshold", "phrases", "phrase_nbest", "phrase_mass", "phrase_threshold",
                                         "phrase_fallback", "hotwords", "hotword_boost") if p[k] is not None})      # (absent: do_whisper takes the settings' values)
        return await loop.run_in_executor(pool, lambda: do_whisper(audio_file, p["model"], p["beam_size"], "transcribe", p["detect_language"],
                                                                   p["force_language"], p["translate"], models=get_models(), **kw))

    def bad(msg):
        return JSONResponse(content={"error": msg}, status_code=400)

    def get_sv():
        with sv_lock:
            if state["sv"] is None:
                from .sv import SpeakerVerifier
                state["sv"] = SpeakerVerifier(s.sv_model_path)
            return state["sv"]

    async def run_sv(audio_file):
        from .sv import do_sv
        loop = asyncio.get_running_loop()
        return await loop.run_in_executor(pool, lambda: do_sv(audio_file, s.sv_threshold, get_sv(), s.sv_speakers_dir,
                                                               resample_on_gpu=getattr(s, "resample_on_gpu", False)))

    @app.get("/api/ping")
    async def ping():
        return JSONResponse(content={"message": "pong"})

    @app.post("/api/asr")
    async def asr(request: Request):
        try:
            p = params(request)
        except BadRequest as e:
            return bad(str(e))
        if p["force_language"] and not check_model_language(p["force_language"], p["model"]):
            return bad("Invalid force_language")
        try:
            data = parse_multipart(await request.body(), request.headers.get("content-type"))
            res = await run_whisper(io.BytesIO(data), p)
        except InvalidAudio as e:
            logger.debug("ASR: %s - returning HTTP 400", e)
            return bad("Invalid audio")
        except ValueError as e:        # malformed upload / unknown model (the reference lets these surface as 500s)
            return bad(str(e))
        language, text, infer_time, translation, infer_speedup, audio_duration = res
        out = {"infer_time": infer_time, "infer_speedup": infer_speedup, "audio_duration": audio_duration, "language": language, "text": text}
        if translation:
            out["translation"] = translation
        if p["timestamps"] or p["word_timestamps"]:
            out["segments"] = res.segments
        if getattr(res, "matches", None) is not None:      # a phrase-constrained request: the ranked phrases
            out["matches"] = _json_matches(res.matches)
            if getattr(res, "matched", None) is not None:      # (a request with a phrase_threshold)
                out["matched"] = bool(res.matched)
        return JSONResponse(content=out)

    @app.post("/api/willow")
    async def willow(request: Request):
        try:
            p = params(request)
        except BadRequest as e:
            return bad(str(e))
        q = request.query_params
        save_audio, stats, voice_auth = _as_bool(q.get("save_audio"), False), _as_bool(q.get("stats"), False), _as_bool(q.get("voice_auth"), False)
        if p["force_language"] and not check_model_language(p["force_language"], p["model"]):
            return bad("Invalid force_language")
        if voice_auth and not s.support_sv:
            return bad("voice_auth (speaker verification) is disabled (support_sv)")
        h = request.headers
        sample_rate, bits, channel = h.get("x-audio-sample-rate", "").lower(), h.get("x-audio-bits", "").lower(), h.get("x-audio-channel", "").lower()
        codec = h.get("x-audio-codec", "").lower()
        chunks = []
        async for chunk in request.stream():
            chunks.append(chunk)
        body = b"".join(chunks)
        try:
            if codec == "pcm":
                audio_file = write_stream_wav(body, int(sample_rate), int(bits), int(channel))
            elif codec in ("wav", "flac"):
                audio_file = io.BytesIO(body)
            else:
                raise InvalidAudio(f"codec {codec!r} needs PyAV")
            if save_audio:
                path = os.environ.get("WIS_SAVE_AUDIO_PATH", "nginx/static/audio/willow.wav")
                os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
                with open(path, "wb") as f:
                    f.write(audio_file.getbuffer())
            sv_results, speaker_status = None, None
            if voice_auth:       # main.py:1324-1336: before Whisper; stats forced on
                stats = True
                try:
                    sv_results = await run_sv(audio_file)
                except ValueError as e:     # undecodable audio -> 400 "Invalid audio" below
                    raise InvalidAudio(str(e)) from e
                if not sv_results:
                    logger.debug("WILLOW: Unknown or unauthorized voice - returning HTTP 406")
                    return PlainTextResponse("Unauthorized voice", status_code=406)
                audio_file.seek(0)
                speaker_status = f"I heard {list(sv_results.keys())[0]} say:"
            res = await run_whisper(audio_file, p)
        except InvalidAudio as e:
            logger.debug("WILLOW: %s - returning HTTP 400", e)
            return bad("Invalid audio")
        except ValueError as e:        # bad x-audio-* header values / unknown model
            return bad("Invalid audio" if "invalid literal" in str(e) else str(e))
        language, text, infer_time, translation, infer_speedup, audio_duration = res
        if stats:
            out = {"infer_time": infer_time, "infer_speedup": infer_speedup, "audio_duration": audio_duration, "language": language, "text": text}
        else:
            out = {"language": language, "text": text}
        if translation:
            out["translation"] = translation
        if p["timestamps"] or p["word_timestamps"]:
            out["segments"] = res.segments
        if getattr(res, "matches", None) is not None:      # a phrase-constrained request: the ranked phrases
            out["matches"] = _json_matches(res.matches)
            if getattr(res, "matched", None) is not None:      # (a request with a phrase_threshold)
                out["matched"] = bool(res.matched)
        if voice_auth:
            out["voice_auth"] = sv_results
            out["speaker_status"] = speaker_status
        return JSONResponse(content=out)

    app.state.wis = state
    app.state.pool = pool
    return app


def _listen_socket(host, port):
    """A listening socket of its own on the SHARED (host, port): SO_REUSEPORT lets every worker process bind the same address and the kernel
    spreads incoming connections over the listeners (by a hash of the connection's addresses) - one port for the node, no proxy process in
    the data path."""
    import socket
    fam = socket.AF_INET6 if ":" in host else socket.AF_INET
    sock = socket.socket(fam, socket.SOCK_STREAM)
    sock.setsockopt(socket.SOL_SOCKET, socket.SO_REUSEADDR, 1)
    sock.setsockopt(socket.SOL_SOCKET, socket.SO_REUSEPORT, 1)
    sock.bind((host, port))
    sock.listen(2048)
    return sock


def _load_factory(spec):
    """'package.module:callable' -> the callable (default: this module's create_app; tests / tools/host_ceiling.py serve a fake-engine app)"""
    import importlib
    mod, _, name = spec.partition(":")
    return getattr(importlib.import_module(mod), name or "create_app")


def serve_worker(args):
    """One server process of a node (spawned by `supervise`): sees ONE GPU (the parent set HIP_VISIBLE_DEVICES before this interpreter
    started, so device 0 here is the node's device `args.device`), listens on the shared port, drains on SIGTERM (uvicorn: stops accepting,
    finishes the requests in flight)."""
    import uvicorn
    app = _load_factory(args.app)()
    config = uvicorn.Config(app, log_level=args.log_level, timeout_graceful_shutdown=args.graceful_timeout, timeout_keep_alive=3600,
                            forwarded_allow_ips=os.environ.get("FORWARDED_ALLOW_IPS", "127.0.0.1"))
    logger.info("worker %d: GPU %s, pid %d, %s:%d", args.worker_index, os.environ.get("HIP_VISIBLE_DEVICES", "all"), os.getpid(), args.host, args.port)
    uvicorn.Server(config).run(sockets=[_listen_socket(args.host, args.port)])


def supervise(args, devices):
    """`--workers-per-node N`: N server processes behind ONE port - the deployment that serves a node (utterances shard over
    the GPUs with no exchange; reference main.py:295 `device_index=[*range(n)]` inside one gunicorn worker, entrypoint.sh:19-21).  One Python
    process answers 370-390 requests/s (tools/host_ceiling.py: ASGI + multipart + FLAC decode + batching under the GIL), an MI355X decodes
    ~170 utterances/s of the jmeter shape, so ONE process cannot feed eight GPUs: each GPU gets a process of its own (its model replicas, its
    micro-batcher, its thread pool), pinned with HIP_VISIBLE_DEVICES, all listening on the same address with SO_REUSEPORT.  This parent only
    supervises: it restarts a worker that dies (three times, then gives the node up), forwards SIGTERM / SIGINT and waits `--graceful-timeout`
    seconds for the workers to drain before it kills what is left (the reference's gunicorn flags: --graceful-timeout 10)."""
    import signal
    import subprocess
    import sys
    import time
    n = args.workers_per_node
    base = [sys.executable, "-m", "wis_hip.server", "--host", args.host, "--port", str(args.port), "--log-level", args.log_level, "--app", args.app,
            "--graceful-timeout", str(args.graceful_timeout)]
    procs, restarts, stopping = {}, {}, []

    def spawn(i):
        env = dict(os.environ)
        if devices:
            env["HIP_VISIBLE_DEVICES"] = str(devices[i % len(devices)])
        env["WIS_WORKER_INDEX"] = str(i)
        procs[i] = subprocess.Popen(base + ["--worker-index", str(i)], env=env)

    def stop(signum, _frame):
        stopping.append(signum)

    signal.signal(signal.SIGTERM, stop)
    signal.signal(signal.SIGINT, stop)
    for i in range(n):
        spawn(i)
    logger.info("supervisor pid %d: %d worker processes on %s:%d (GPUs %s)", os.getpid(), n, args.host, args.port, devices or "unpinned")
    rc = 0
    while not stopping:
        time.sleep(0.2)
        for i, p in list(procs.items()):
            if p.poll() is not None and not stopping:
                restarts[i] = restarts.get(i, 0) + 1
                logger.warning("worker %d (pid %d) exited with %s", i, p.pid, p.returncode)
                if restarts[i] > 3:
                    logger.error("worker %d keeps dying: shutting the node down", i)
                    stopping.append(signal.SIGTERM)
                    rc = 1
                    break
                spawn(i)
    for p in procs.values():
        if p.poll() is None:
            p.send_signal(signal.SIGTERM)
    deadline = time.time() + args.graceful_timeout + 2
    for p in procs.values():
        try:
            p.wait(max(0.1, deadline - time.time()))
        except subprocess.TimeoutExpired:
            p.kill()
    return rc


def main(argv=None):
    """`python -m wis_hip.server [--host 0.0.0.0] [--port 19000] [--workers-per-node N]` - the reference serves on 19000 behind nginx
    (entrypoint.sh:19-21, nginx.conf:99-103).  N > 1: one server process per GPU behind the one port (supervise)."""
    import argparse
    import uvicorn
    ap = argparse.ArgumentParser(description="Willow Inference Server ASR endpoints over the MI355X HIP path")
    ap.add_argument("--host", default="0.0.0.0")
    ap.add_argument("--port", type=int, default=19000)
    ap.add_argument("--log-level", default=os.environ.get("LOG_LEVEL", "info"))
    ap.add_argument("--workers-per-node", type=int, default=1, help="server processes behind the one port: one per GPU (0 = one per visible GPU)")
    ap.add_argument("--devices", default="", help="comma-separated GPU ids the workers are pinned to, round-robin (default: 0 .. workers-1)")
    ap.add_argument("--graceful-timeout", type=int, default=10, help="seconds a worker may take to finish the requests in flight on SIGTERM")
    ap.add_argument("--app", default="wis_hip.server:create_app", help="module:factory of the ASGI app the workers serve")
    ap.add_argument("--worker-index", type=int, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args(argv)
    logging.basicConfig(level=getattr(logging, args.log_level.upper(), logging.INFO))
    if args.worker_index is not None:
        return serve_worker(args)
    n = args.workers_per_node
    if n == 0:
        from . import _lib
        n = args.workers_per_node = max(1, _lib.device_count())
    if n > 1:
        devices = [int(d) for d in args.devices.split(",") if d.strip()] or list(range(n))
        raise SystemExit(supervise(args, devices))
    uvicorn.run(_load_factory(args.app)(), host=args.host, port=args.port, log_level=args.log_level)


if __name__ == "__main__":
    main()
