"""MI355X build of the part of `GANsynth_pytorch` the reference calls (the package itself is absent
from the reference tree and un-pinned): `spectrograms_helper.{SpectrogramsHelper, MelSpectrogramsHelper}`, with the
RIFF reader (`wavfile`) and the sample-rate converter (`resample`) behind `from_wavfile`."""
