"""Projection encoders (``u_net_like_encoder``) and the autoencoders that pair them with a generator (``autoencoder``); reference:
networks/encoder/.  Nothing is imported here: ``networks`` needs the autoencoder classes only, the encoders (and with them the
kernel library) load where they are built."""
