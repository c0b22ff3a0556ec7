"""Host drivers of the reference's experiments (myriad/experiments/) whose hot path runs on the device."""
