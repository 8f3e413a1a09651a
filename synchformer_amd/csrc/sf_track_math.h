// The scalar arithmetic the track read-outs share: sf_track.hip (the chains with one lane per state) and sf_track_wide.hip (the wide chain, one thread per state).
// One statement each, so that the gate's term and the (-inf) - (-inf) guard are the same bits wherever a read-out uses them.
#pragma once
#include "sf_common.h"
#include <cmath>

// m where it is finite, 0 otherwise (false for NaN too): the subtrahend of every subtraction that could meet (-inf) - (-inf).
__device__ __forceinline__ float fb_finite_or_zero(float m) { return (m > -INFINITY && m < INFINITY) ? m : 0.f; }

// softplus(x) = log(1 + exp(x)) without overflow: -softplus(-d) = log sigmoid(d).
__device__ __forceinline__ float gate_softplus(float x) { return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))); }
