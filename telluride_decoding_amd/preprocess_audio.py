"""Drop-in for the reference's preprocess_audio (preprocess_audio.py): stores that take audio in blocks
of any length and yield one number per fixed window.  Each window is a small NumPy reduction on the host
(a device launch per window would only add latency)."""
import numpy as np

from telluride_decoding_amd import result_store


class AudioIntensityStore(result_store.WindowedDataStore):
  """Process a window of data, calculating the mean-squared value."""

  def next_window(self):
    for win in super(AudioIntensityStore, self).next_window():
      yield np.mean(np.square(win))


class AudioLoudnessMick(result_store.WindowedDataStore):
  """Process a window of data, using Mick's loudness approximation: the mean of |x|^log10(2)."""

  def next_window(self):
    for audio_data in super(AudioLoudnessMick, self).next_window():
      yield np.mean(np.abs(audio_data) ** np.log10(2))
