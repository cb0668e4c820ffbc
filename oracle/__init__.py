"""CPU ORACLE — TEST INFRASTRUCTURE ONLY.

This package restates the reference algorithm for the hot path
(TheCacophonyProject/audio-training: custommel.py, tfdataset.py normalize /
mix_up / raw_to_mel, predict_utils.get_spect, tfpcen.py, resnet/wr_resnet*.py,
audiomodel.loss / optimizer) on the CPU so that the HIP path can be checked.

Only `tests/`, `__graft_entry__.smoke()` and the `cpu_baseline` leg of
`bench.py` may import it, and only as the checker / the reported CPU baseline.
The product path (`audio-training_amd/`) never imports it and fails loudly when
its HIP library is missing.

Parity pinning:
  * `mel_f` / `mel_spec` are pinned bit-for-bit against golden vectors produced
    by the reference `custommel.py` itself (oracle/gen_golden.py ->
    tests/golden/mel_f_*.npz, mel_spec_p*.npz).
  * The streaming path's index work -- identifytracks.merge_signals /
    get_tracks_from_signals / Signal / get_end's chunk scan and
    predict_utils.load_samples' window cutting -- is pinned bit-for-bit
    against tests/golden/tracks_golden.npz, produced by the reference modules
    themselves (oracle/gen_golden_tracks.py, stub librosa / cv2 / tensorflow
    imports that those functions never call).
  * STFT (tf.signal.stft pad_end, librosa.stft center), PCEN, LME, Keras layer
    semantics and Adam live in third-party libraries (tensorflow, tfp,
    librosa, keras -- unpinned in requirements.txt:1-13) that are absent from
    this image; they are restated from their published definitions and are
    "parity unpinned" beyond the golden mel filterbank.
  * `torch_ref.pcen_torch` follows TF at the clamp edges: MinimumGrad /
    MaximumGrad give the whole gradient to gain / root at exactly 1.0 (and
    none beyond), clip_by_value passes it on [0, 1]; amax / amin share it
    among tied extrema (tests/test_frontend_cases.py).
  * `frontend_cases` is the table of front-end edge cases (PCEN shapes around
    the 64-row workgroup and the 32-step chunk, ten parameter sets, per-probe
    gradients; mel plans with odd / single / long / empty / DC / Nyquist
    bands; n_fft 2048 / 512 / 256).  Its conditions hold on the reference
    alone (measured: gap under the maximum >= 2.2e-4 of the range, weakest
    probe 1.25e-3 of the strongest, float32 noise of the reference
    <= 6.1e-4 * s); the kernels measure <= 1.9e-6 (PCEN output),
    <= 6.5e-4 * s (gradients, bound 2e-3 * s) and <= 8.4e-7 (mel, bound
    2e-5) against it (tests/test_frontend_edges_gpu.py).
"""
