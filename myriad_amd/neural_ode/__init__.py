"""Host side of the reference's myriad/neural_ode/: training of the network system by trajectory matching."""
