"""HTTP surface of the interactive inpainting service (reference flask_server.py): same routes,
query arguments and JSON schema for the operations built on MI355X

  POST /timerange-change?layer=&temperature=&start_index_top=&uniform_sampling=&pitch=&instrument_family_str=
       body {top_code: int[F_t][T], bottom_code: int[F_b][T_b], mask: bool[F][W],
             top_conditioning, bottom_conditioning: {modality: value[F][T]}}          (:685-870,934-1000)
  GET/POST /generate?pitch=&instrument_family_str=&temperature=                         (:376-443)
  POST /erase?eraser_amplitude=&start_index_top=                                        (:873-931)
  POST /get-audio[?fs_hz=]   -> audio/wav (16-bit PCM written with the standard library); `fs_hz` (not in the
       reference) asks for the audio resampled to that rate                               (:1003-1021)
  POST /get-audio-spliced[?fs_hz=]   (not in the reference) multipart: file `audio`, the original upload (as
       /analyze-audio takes it, converted to the models' rate), and `codes`, the JSON /get-audio takes (a form field or a
       file part) -> audio/wav: the upload's own samples wherever the codes are those of the upload, the decoded codes
       where they were edited, phase-locked to the upload at both seams (csrc/spec_splice.hip)
  POST /transpose-audio?semitones= | ?to_pitch= [&preserve_formants=1]   (not in the reference) multipart: file `audio` (as
       /analyze-audio takes it) -> audio/wav at the models' rate: the sound `semitones` higher (fractional and negative
       values too), or at the MIDI pitch `to_pitch` (its own pitch is estimated; 400 when it is unvoiced), at its own
       length; with preserve_formants=1 its resonances stay where they were (csrc/formant.hip)
  POST /shift-formants?semitones=   (not in the reference) multipart: file `audio` -> audio/wav: the sound at its own pitch
       and length, its formants `semitones` higher (GANsynth_pytorch/stretch.py `shift_formants`, csrc/formant.hip)
  POST /stretch-audio?factor=&keep_attack_s=&keep_release_s=   (not in the reference) multipart: file `audio` ->
       audio/wav: the sound `factor` times as long at its own pitch; the first / last seconds named keep their own rate
       (both: GANsynth_pytorch/stretch.py, csrc/stft_stretch.hip; the arguments may also be form fields)
  POST /bend-audio?vibrato_hz=&vibrato_cents= | ?glide_from=&glide_to= | ?flatten=1[&to_pitch=] [&preserve_formants=1]   (not in the reference)
       multipart: file `audio` -> audio/wav at its own length: a vibrato added, a glide between two transpositions in
       semitones, or the sound's own vibrato and drift removed and the sound tuned to the MIDI pitch `to_pitch` (its own
       rounded pitch by default; 400 when it is unvoiced)   (GANsynth_pytorch/bend.py, csrc/warp_resample.hip)
  POST /analyze-audio?pitch=&instrument_family_str=   multipart file `audio` (RIFF / PCM 16-bit or float32, mono or
       averaged to mono, at any sampling rate the resampler takes -- 44.1 and 48 kHz recordings are converted to
       the models' rate on the GPU, GANsynth_pytorch/resample.py; read with the standard library)  (:557-568,624-667)
       without `pitch`, or with `pitch=auto` (not in the reference): the pitch is estimated from the sound on the GPU
       (GANsynth_pytorch/pitch.py) and fills the conditioning maps; 400 when the sound has none (noise, silence)
  POST /top-conditioned-sample?instrument_family_str=&min_pitch=&max_pitch=&temperature=&top_p=&top_k=
       body {top_code, bottom_code} -> application/zip of `{family}-{pitch}.wav`, one per pitch             (:1049-1115)
  GET/POST /sample-from-dataset?duration_top=&pitch=&pitch_class=&octave=&instrument_family_str=
       a stored codemap pair meeting the constraints (`codes_dataset`: the LMDB code database or any
       sequence of its items; 404 when nothing matches -- the reference searches for ever)                 (:333-372,446-514)
       POST ...&nearest=1 with body {top_code, bottom_code} (not in the reference; needs `codes_index`): the stored
       pair NEAREST to that sound among those meeting the constraints (utils/datasets/code_index.py)
  GET/POST /test-generate?pitch=&instrument_family_str=   uniformly random codemaps                         (:517-552)
  POST /get-spectrogram-image   body {top_code, bottom_code} -> image/png (viridis, standard library)       (:1024-1046)
  response {top_code, bottom_code, top_conditioning, bottom_conditioning}               (:991-1000)

A thin adapter: parsing / serialisation here, all compute in `inpainting.py`.  The models (and the
code database) are handed to `create_app` already loaded: checkpoint paths are deployment plumbing.
Global (non-local) class conditioning only, like the reference's default deployment.
"""
from __future__ import annotations

import io
import json
import math
import struct
import zipfile
from typing import Mapping, Optional

import flask
import torch

import inpainting
from GANsynth_pytorch import resample as _resample
from GANsynth_pytorch.wavfile import read_wav


def _wav_bytes(audio: torch.Tensor, fs_hz: int) -> bytes:
    pcm = (audio.clamp(-1, 1) * 32767.0).round().to(torch.int16).cpu().numpy().tobytes()
    header = b"RIFF" + struct.pack("<I", 36 + len(pcm)) + b"WAVEfmt " + struct.pack(
        "<IHHIIHH", 16, 1, 1, fs_hz, fs_hz * 2, 2, 16) + b"data" + struct.pack("<I", len(pcm))
    return header + pcm


def _read_wav(data: bytes):
    """RIFF/WAVE bytes -> (float32 mono tensor in [-1, 1], sampling rate): `GANsynth_pytorch.wavfile.read_wav`."""
    return read_wav(data)


def create_app(vqvae, transformer_top, transformer_bottom, label_encoders_per_modality: Mapping[str, object],
               device, spectrograms_helper=None, top_k: int = 0, top_p: float = 0.0,
               seed: Optional[int] = None, max_sound_duration_s: float = 4.0, codes_dataset=None,
               spectrograms_upsampling_factor: int = 1, codes_index=None) -> flask.Flask:
    """`label_encoders_per_modality[name].transform([value]) -> [class index]` (sklearn LabelEncoder
    in the reference, `utils/datasets/label_encoders.py`).  codes_index: a `utils.datasets.code_index.CodeIndex` of the
    code database, for the `nearest=1` form of /sample-from-dataset."""
    app = flask.Flask(__name__)
    device = torch.device(device)
    generator = torch.Generator().manual_seed(seed) if seed is not None else None
    sampling = dict(top_k_sampling_k=top_k, top_p_sampling_p=top_p)

    def conditioning_tensors(args) -> Mapping[str, torch.Tensor]:
        values = {'pitch': args.get('pitch', type=int), 'instrument_family_str': str(args.get('instrument_family_str'))}
        return {name: torch.as_tensor(label_encoders_per_modality[name].transform([value])).long().reshape(1, 1)
                for name, value in values.items()}, values

    def codes(json_data):
        return (torch.LongTensor(json_data['top_code']).unsqueeze(0).to(device),
                torch.LongTensor(json_data['bottom_code']).unsqueeze(0).to(device))

    def respond(top_code, bottom_code, conditioning_top, conditioning_bottom):
        return flask.jsonify({'top_code': top_code[0].int().cpu().numpy().tolist(),
                              'bottom_code': bottom_code[0].int().cpu().numpy().tolist(),
                              'top_conditioning': conditioning_top, 'bottom_conditioning': conditioning_bottom})

    def matrix(shape, value):
        return [[value] * shape[1]] * shape[0]

    @app.route('/generate', methods=['GET', 'POST'])
    def generate():
        args = flask.request.args
        cls, values = conditioning_tensors(args)
        top, bottom = inpainting.generate(transformer_top, transformer_bottom, float(args.get('temperature')), cls, cls,
                                          device, generator=generator, **sampling)
        return respond(top, bottom, {k: matrix(transformer_top.shape, v) for k, v in values.items()},
                       {k: matrix(transformer_bottom.shape, v) for k, v in values.items()})

    @app.route('/timerange-change', methods=['POST'])
    def timerange_change():
        args = flask.request.args
        json_data = flask.request.get_json(force=True)
        cls, values = conditioning_tensors(args)
        top_code, bottom_code = codes(json_data)
        mask = torch.BoolTensor(json_data['mask']).unsqueeze(0)
        layer = str(args.get('layer'))
        uniform = str(args.get('uniform_sampling', default='False')).lower() in ('1', 'true', 'yes', 'y', 'on', 't')
        new_top, new_bottom = inpainting.timerange_change(
            transformer_top, transformer_bottom, top_code, bottom_code, mask, layer,
            args.get('start_index_top', type=int), args.get('temperature', type=float), cls, cls, device,
            uniform_sampling=uniform, generator=generator, **sampling)
        cond_top, cond_bottom = json_data.get('top_conditioning'), json_data.get('bottom_conditioning')
        if layer == 'top' and cond_bottom is not None:
            # the regenerated zone now carries the requested classes (flask_server.py:845-853)
            ratio_f = transformer_bottom.shape[0] // transformer_top.shape[0]
            ratio_t = transformer_bottom.shape[1] // transformer_top.shape[1]
            m = mask[0].repeat_interleave(ratio_f, 0).repeat_interleave(ratio_t, 1).tolist()
            cond_bottom = {name: [[values[name] if mv else pv for pv, mv in zip(row, mrow)]
                                  for row, mrow in zip(rows, m)] for name, rows in cond_bottom.items()}
        return respond(new_top, new_bottom, cond_top, cond_bottom)

    @app.route('/erase', methods=['POST'])
    def erase():
        args = flask.request.args
        json_data = flask.request.get_json(force=True)
        top_code, bottom_code = codes(json_data)
        new_top, new_bottom = inpainting.erase(vqvae, top_code, bottom_code, torch.BoolTensor(json_data['mask']),
                                               float(args.get('eraser_amplitude')), int(args.get('start_index_top')))
        return respond(new_top, new_bottom, json_data.get('top_conditioning'), json_data.get('bottom_conditioning'))

    @app.route('/get-audio', methods=['POST'])
    def get_audio():
        if spectrograms_helper is None:
            flask.abort(501)
        top_code, bottom_code = codes(flask.request.get_json(force=True))
        audio = inpainting.codes_to_audio(vqvae, spectrograms_helper, top_code, bottom_code)[0]
        fs_hz = flask.request.args.get('fs_hz', type=int, default=None)
        if fs_hz is None:
            fs_hz = spectrograms_helper.fs_hz
        else:
            try:
                audio = _resample.resample(audio, spectrograms_helper.fs_hz, fs_hz)
            except ValueError as e:
                flask.abort(400, description=str(e))
        return flask.send_file(io.BytesIO(_wav_bytes(audio, fs_hz)), mimetype="audio/wav", max_age=0)

    def uploaded_audio():
        """the multipart file `audio` as mono samples at the models' rate; 400 when it is missing or unreadable"""
        try:
            audio, rate = _read_wav(flask.request.files['audio'].read())
        except (KeyError, ValueError, struct.error) as e:
            flask.abort(400, description=str(e))
        if rate != spectrograms_helper.fs_hz:
            # flask_server.py:557-568,644-649: the upload is converted to the models' rate.  Only what survives the trim
            # to max_sound_duration_s is converted (the filter reaches `width` input samples past an output's instant)
            try:
                _, _, width, _ = _resample.geometry(rate, spectrograms_helper.fs_hz)
                audio = audio[:int(max_sound_duration_s * rate) + 2 * width]
                audio = _resample.resample(audio.to(device), rate, spectrograms_helper.fs_hz)
            except ValueError as e:
                flask.abort(400, description=str(e))
        return audio

    @app.route('/get-audio-spliced', methods=['POST'])
    def get_audio_spliced():
        if spectrograms_helper is None:
            flask.abort(501)
        original = uploaded_audio()
        try:
            part = flask.request.files.get('codes')
            text = part.read() if part is not None else flask.request.form['codes']
            top_code, bottom_code = codes(json.loads(text))
        except (KeyError, ValueError, TypeError) as e:
            flask.abort(400, description=f"codes: {e}")
        audio = inpainting.codes_to_audio_spliced(vqvae, spectrograms_helper, original, top_code, bottom_code)[0]
        fs_hz = flask.request.args.get('fs_hz', type=int, default=None)
        if fs_hz is None:
            fs_hz = spectrograms_helper.fs_hz
        else:
            try:
                audio = _resample.resample(audio, spectrograms_helper.fs_hz, fs_hz)
            except ValueError as e:
                flask.abort(400, description=str(e))
        return flask.send_file(io.BytesIO(_wav_bytes(audio, fs_hz)), mimetype="audio/wav", max_age=0)

    def number(name, default=None):
        """a numeric argument from the query string or the form; 400 when it is not a number"""
        text = flask.request.values.get(name)
        if text is None:
            return default
        try:
            return float(text)
        except ValueError:
            flask.abort(400, description=f"{name}: not a number: {text!r}")

    @app.route('/transpose-audio', methods=['POST'])
    def transpose_audio():
        if spectrograms_helper is None:
            flask.abort(501)
        semitones, to_pitch = number('semitones'), number('to_pitch')
        if (semitones is None) == (to_pitch is None):
            flask.abort(400, description="give exactly one of semitones and to_pitch")
        keep = dict(preserve_formants=True) if number('preserve_formants', 0.0) != 0.0 else {}
        original = uploaded_audio()
        try:
            audio, _, _ = inpainting.transpose_sound(vqvae, spectrograms_helper, original.to(device), semitones=semitones,
                                                     to_pitch=to_pitch, re_encode=False, **keep)
        except ValueError as e:
            flask.abort(400, description=str(e))
        return flask.send_file(io.BytesIO(_wav_bytes(audio.reshape(-1), spectrograms_helper.fs_hz)), mimetype="audio/wav",
                               max_age=0)

    @app.route('/shift-formants', methods=['POST'])
    def shift_formants():
        if spectrograms_helper is None:
            flask.abort(501)
        semitones = number('semitones')
        if semitones is None:
            flask.abort(400, description="semitones is missing")
        if not math.isfinite(semitones) or abs(semitones) > 24.0:
            flask.abort(400, description=f"semitones must be finite and within +-24, got {semitones}")
        original = uploaded_audio()
        try:
            audio, _, _ = inpainting.shift_formants_sound(vqvae, spectrograms_helper, original.to(device), semitones,
                                                          re_encode=False)
        except ValueError as e:
            flask.abort(400, description=str(e))
        return flask.send_file(io.BytesIO(_wav_bytes(audio.reshape(-1), spectrograms_helper.fs_hz)), mimetype="audio/wav",
                               max_age=0)

    @app.route('/bend-audio', methods=['POST'])
    def bend_audio():
        if spectrograms_helper is None:
            flask.abort(501)
        vib, gl = (number('vibrato_hz'), number('vibrato_cents')), (number('glide_from'), number('glide_to'))
        flatten, to_pitch = number('flatten', 0.0) != 0.0, number('to_pitch')
        for pair, names in ((vib, "vibrato_hz and vibrato_cents"), (gl, "glide_from and glide_to")):
            if (pair[0] is None) != (pair[1] is None):
                flask.abort(400, description=f"{names} come together")
        if (vib[0] is not None) + (gl[0] is not None) + flatten != 1:
            flask.abort(400, description="give exactly one of vibrato_hz + vibrato_cents, glide_from + glide_to and flatten=1")
        if to_pitch is not None and not flatten:
            flask.abort(400, description="to_pitch belongs to flatten=1")
        keep = dict(preserve_formants=True) if number('preserve_formants', 0.0) != 0.0 else {}
        original = uploaded_audio()
        try:
            audio, _, _ = inpainting.bend_sound(vqvae, spectrograms_helper, original.to(device),
                                                vibrato=vib if vib[0] is not None else None,
                                                glide=gl if gl[0] is not None else None, flatten=flatten, to_pitch=to_pitch,
                                                re_encode=False, **keep)
        except ValueError as e:
            flask.abort(400, description=str(e))
        return flask.send_file(io.BytesIO(_wav_bytes(audio.reshape(-1), spectrograms_helper.fs_hz)), mimetype="audio/wav",
                               max_age=0)

    @app.route('/stretch-audio', methods=['POST'])
    def stretch_audio():
        if spectrograms_helper is None:
            flask.abort(501)
        factor = number('factor')
        if factor is None:
            flask.abort(400, description="factor is missing")
        keep_attack_s, keep_release_s = number('keep_attack_s', 0.0), number('keep_release_s', 0.0)
        original = uploaded_audio()
        try:
            audio = inpainting.stretch_sound(vqvae, spectrograms_helper, audio=original.to(device), factor=factor,
                                             keep_attack_s=keep_attack_s, keep_release_s=keep_release_s)
        except ValueError as e:
            flask.abort(400, description=str(e))
        return flask.send_file(io.BytesIO(_wav_bytes(audio.reshape(-1), spectrograms_helper.fs_hz)), mimetype="audio/wav",
                               max_age=0)

    @app.route('/analyze-audio', methods=['POST'])
    def analyze_audio():
        if spectrograms_helper is None:
            flask.abort(501)
        args = flask.request.args
        values = {'pitch': args.get('pitch', type=int), 'instrument_family_str': str(args.get('instrument_family_str'))}
        audio = uploaded_audio()
        res_n = inpainting.top_resolution_n(vqvae, transformer_top, transformer_bottom, spectrograms_helper, device)
        duration_n = inpainting.adapt_duration(audio.numel(), spectrograms_helper.fs_hz, max_sound_duration_s, res_n,
                                               transformer_top.shape[1])
        if args.get('pitch') in (None, 'auto'):
            # nobody knows the pitch of an upload: estimated from the samples about to be encoded (GANsynth_pytorch/pitch.py)
            encoder = label_encoders_per_modality['pitch']
            values['pitch'], _ = inpainting.estimate_pitch(
                audio[:duration_n].to(device), spectrograms_helper,
                pitch_range=getattr(encoder, 'classes_', getattr(encoder, 'classes', None)))
            if values['pitch'] is None:
                flask.abort(400, description="no pitch found in the sound (noise or silence): give the `pitch` argument")
        top_code, bottom_code = inpainting.analyze_audio(vqvae, spectrograms_helper, audio, duration_n, device)
        return respond(top_code, bottom_code, {k: matrix(transformer_top.shape, v) for k, v in values.items()},
                       {k: matrix(transformer_bottom.shape, v) for k, v in values.items()})

    @app.route('/top-conditioned-sample', methods=['POST'])
    def top_conditioned_sample():
        if spectrograms_helper is None:
            flask.abort(501)
        args = flask.request.args
        top_code, _ = codes(flask.request.get_json(force=True))
        family = str(args.get('instrument_family_str'))
        lo, hi = args.get('min_pitch', type=int), args.get('max_pitch', type=int)
        if lo is None or hi is None or not lo < hi:
            flask.abort(400, description="Provide increasing range for range conditioning")
        cls = {'pitch': torch.as_tensor(label_encoders_per_modality['pitch'].transform(list(range(lo, hi)))).long(),
               'instrument_family_str': torch.as_tensor(
                   label_encoders_per_modality['instrument_family_str'].transform([family])).long()}
        _, audio = inpainting.top_conditioned_sample(
            vqvae, transformer_bottom, spectrograms_helper, top_code, float(args.get('temperature')), cls, device,
            top_k_sampling_k=int(args.get('top_k') or 0), top_p_sampling_p=float(args.get('top_p') or 0.0),
            generator=generator)
        buf = io.BytesIO()
        with zipfile.ZipFile(buf, 'w') as zf:        # (in memory: the reference writes sample files and a zip to its upload folder)
            for pitch, row in zip(range(lo, hi), audio):
                zf.writestr(f'{family}-{pitch}.wav', _wav_bytes(row, spectrograms_helper.fs_hz))
        buf.seek(0)
        return flask.send_file(buf, mimetype="application/zip", max_age=0)

    @app.route('/sample-from-dataset', methods=['GET', 'POST'])
    def sample_from_dataset():
        args = flask.request.args
        nearest = flask.request.method == 'POST' and \
            str(args.get('nearest', default='')).lower() in ('1', 'true', 'yes', 'y', 'on', 't')
        if (codes_index if nearest else codes_dataset) is None:
            flask.abort(501)
        constraints = {}
        pitch = args.get('pitch', type=int, default=None)
        if pitch is not None:
            constraints['pitch'] = pitch
        pitch_class = args.get('pitch_class', type=int, default=None)
        if pitch_class is not None and 0 <= pitch_class <= 12:
            constraints['pitch_class'] = pitch_class
        octave = args.get('octave', type=int, default=None)
        if octave is not None and octave >= 0:
            constraints['octave'] = octave
        family = args.get('instrument_family_str', type=str, default=None)
        if family is not None:
            constraints['instrument_family_str'] = family
        try:
            if nearest:
                (top, bottom), attributes = inpainting.sample_from_database(
                    codes_dataset, label_encoders_per_modality, args.get('duration_top', type=int), constraints,
                    similar_to=codes(flask.request.get_json(force=True)), index=codes_index)
            else:
                (top, bottom), attributes = inpainting.sample_from_database(
                    codes_dataset, label_encoders_per_modality, args.get('duration_top', type=int), constraints, generator)
        except LookupError as e:
            flask.abort(404, description=str(e))
        values = {'pitch': int(attributes['pitch']), 'instrument_family_str': str(attributes['instrument_family_str'])}
        return respond(top, bottom, {k: matrix(top.shape[1:], v) for k, v in values.items()},
                       {k: matrix(bottom.shape[1:], v) for k, v in values.items()})

    @app.route('/test-generate', methods=['GET', 'POST'])
    def test_generate():
        args = flask.request.args
        values = {'pitch': int(args.get('pitch')), 'instrument_family_str': str(args.get('instrument_family_str'))}
        top = torch.randint(0, vqvae.n_embed_t, (1,) + tuple(transformer_top.shape), generator=generator)
        bottom = torch.randint(0, vqvae.n_embed_b, (1,) + tuple(transformer_bottom.shape), generator=generator)
        return respond(top, bottom, {k: matrix(transformer_top.shape, v) for k, v in values.items()},
                       {k: matrix(transformer_bottom.shape, v) for k, v in values.items()})

    @app.route('/get-spectrogram-image', methods=['POST'])
    def get_spectrogram_image():
        top_code, bottom_code = codes(flask.request.get_json(force=True))
        png = inpainting.spectrogram_png(vqvae, top_code, bottom_code, spectrograms_upsampling_factor)
        return flask.send_file(io.BytesIO(png), mimetype="image/png", max_age=0)

    return app
