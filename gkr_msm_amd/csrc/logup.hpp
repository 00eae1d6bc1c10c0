// LogupMainphaseProtocol (pushforward/logup_mainphase.rs) shared between the provers (prover.hip), the fraction-tree builder and
// the lookup helpers (logup.hip) and the verifier (verifier.hip).  Not part of the ABI.
#pragma once
#include <memory>
#include <vector>

#include "common.hpp"
#include "fr.hip.h"

namespace gm {

#define GM_LOGUP_MAX_INPUTS 64
#define GM_LOGUP_MAX_LOGSIZE 30

// LogupMainphaseProtocol::new (logup_mainphase.rs:75-80): the asserts of the reference plus the size bounds of this library, in one
// host pass; the prover and the verifier share it
inline int32_t logup_shape_check(const uint32_t* logsizes, uint32_t n_inputs) {
    GM_REQUIRE(logsizes, "logup: null logsizes");
    GM_REQUIRE(n_inputs >= 2, "logup: %u inputs, at least 2 are required (logup_mainphase.rs:79)", n_inputs);
    GM_REQUIRE(n_inputs <= GM_LOGUP_MAX_INPUTS, "logup: %u inputs, at most %d are supported", n_inputs, GM_LOGUP_MAX_INPUTS);
    for (uint32_t i = 0; i < n_inputs; i++)
        GM_REQUIRE(logsizes[i] <= GM_LOGUP_MAX_LOGSIZE, "logup: logsizes[%u] = %u, at most %d is supported", i, logsizes[i],
                   GM_LOGUP_MAX_LOGSIZE);
    for (uint32_t i = 1; i < n_inputs; i++)
        GM_REQUIRE(logsizes[i - 1] >= logsizes[i], "logup: logsizes must be non-increasing (logup_mainphase.rs:76-78): logsizes[%u] = %u < logsizes[%u] = %u",
                   i - 1, logsizes[i - 1], i, logsizes[i]);
    GM_REQUIRE(logsizes[0] == logsizes[1], "logup: the first two logsizes must be equal (logup_mainphase.rs:80): %u != %u", logsizes[0],
               logsizes[1]);
    return GM_OK;
}

struct DevBuf;

// one (numerator, denominator) pair of the fraction tree: an input (the caller's columns), a level, or a HI half of a level
struct LogupFrac {
    const Fr* num = nullptr;
    const Fr* den = nullptr;
    uint64_t len = 0;
    Fr h_num, h_den;   // len == 1: the two values on the host (they are prover messages of the zero-variable layers)
};

// make_witness (logup_mainphase.rs:83-143): `layers` in the reference's order with the top fraction taken off (`total`).
// Owns every level, nothing of the inputs.
struct LogupTree {
    std::vector<uint32_t> logsizes;
    std::vector<LogupFrac> layers;
    std::vector<std::shared_ptr<DevBuf>> own;
    Fr total[2];
};

// inputs[i]: 2^logsizes[i] elements each; the shape must have passed logup_shape_check
int32_t logup_build(const std::vector<LogupFrac>& inputs, const std::vector<uint32_t>& logsizes, LogupTree* tree, hipStream_t s);

}  // namespace gm
