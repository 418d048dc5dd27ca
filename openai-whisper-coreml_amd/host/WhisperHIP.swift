// WhisperHIP.swift -- drop-in replacement for Whisper/Whisper/Whisper.swift of tanmayb123/OpenAI-Whisper-CoreML that
// keeps the reference's surface (`struct Whisper`: init / encode(audio:) / decode(audioFeatures:) / LANGUAGES) and
// swaps the two CoreML models for libwhisper_mi355x.so, loaded with dlopen as BASELINE.json's north star prescribes.
//
// *** NOT COMPILED IN THIS REPOSITORY ***  Neither the build image nor the GPU box has a Swift toolchain (`swift`,
// `swiftc` absent; SURVEY.md section 0), so this file is written against include/whisper_mi355x.h by hand and has never
// been through a compiler.  What IS compiled and tested in its place, call for call:
//   host/lid_main.cpp    the language-ID flow of ContentView.swift:56-63 -> Whisper.swift:23-40 (C++, dlopen)
//   host/multi_main.cpp  all GPUs of the node from one process (wm_multi_*)
//   binding.py           ctypes mirror with these very names, used by every parity test
// On a machine with Swift for Linux: `swiftc -O WhisperHIP.swift stft.swift ... -o whisper` next to the .so.
//
// Unchanged from the reference and still needed: Whisper/Whisper/stft.swift (generateSpectrogram: +200 zeros each side,
// raw-pointer call of `generate_spectrogram`) and bridge.h:11 -- seam #1 keeps its symbol, so link libwhisper_mi355x.so
// where libstft.a was linked (project.pbxproj:18,44) and nothing in stft.swift changes.
import Foundation
#if canImport(Glibc)
import Glibc
#endif

struct WhisperError: Error, CustomStringConvertible {
    let description: String
}

/// Field-for-field `wm_dims` of include/whisper_mi355x.h (openai-whisper's ModelDimensions).
struct wm_dims {
    var n_mels: Int32, n_audio_ctx: Int32, n_audio_state: Int32, n_audio_head: Int32, n_audio_layer: Int32
    var n_vocab: Int32, n_text_ctx: Int32, n_text_state: Int32, n_text_head: Int32, n_text_layer: Int32

    /// `whisper.load_model("small")`, the reference's only model (whisper_to_cml.py:7).
    static let small = wm_dims(n_mels: 80, n_audio_ctx: 1500, n_audio_state: 768, n_audio_head: 12, n_audio_layer: 12,
                               n_vocab: 51865, n_text_ctx: 448, n_text_state: 768, n_text_head: 12, n_text_layer: 12)
    static let largeV2 = wm_dims(n_mels: 80, n_audio_ctx: 1500, n_audio_state: 1280, n_audio_head: 20, n_audio_layer: 32,
                                 n_vocab: 51865, n_text_ctx: 448, n_text_state: 1280, n_text_head: 20, n_text_layer: 32)
}

struct Whisper {
    // Whisper.swift:12, unchanged (99 codes, openai-whisper tokenizer order)
    static let LANGUAGES = ["en", "zh", "de", "es", "ru", "ko", "fr", "ja", "pt", "tr", "pl", "ca", "nl", "ar", "sv", "it",
                            "id", "hi", "fi", "vi", "iw", "uk", "el", "ms", "cs", "ro", "da", "hu", "ta", "no", "th", "ur",
                            "hr", "bg", "lt", "la", "mi", "ml", "cy", "sk", "te", "fa", "lv", "bn", "sr", "az", "sl", "kn",
                            "et", "mk", "br", "eu", "is", "hy", "ne", "mn", "bs", "kk", "sq", "sw", "gl", "mr", "pa", "si",
                            "km", "sn", "yo", "so", "af", "oc", "ka", "be", "tg", "sd", "gu", "am", "yi", "lo", "uz", "fo",
                            "ht", "ps", "tk", "nn", "mt", "sa", "lb", "my", "bo", "tl", "mg", "as", "tt", "haw", "ln", "ha",
                            "ba", "jw", "su"]

    private let lib: UnsafeMutableRawPointer
    private let ctx: OpaquePointer
    private let dims: wm_dims

    // C function types of include/whisper_mi355x.h
    private typealias CreateFn = @convention(c) (UnsafePointer<wm_dims>, Int32, UnsafeMutablePointer<OpaquePointer?>) -> Int32
    private typealias LoadFn = @convention(c) (OpaquePointer, UnsafePointer<CChar>) -> Int32
    private typealias CtxFn = @convention(c) (OpaquePointer) -> Int32
    private typealias DestroyFn = @convention(c) (OpaquePointer) -> Void
    private typealias EncodeFn = @convention(c) (OpaquePointer, UnsafePointer<Float>, Int32, UnsafeMutablePointer<Float>, Int32) -> Int32
    private typealias LangFn = @convention(c) (OpaquePointer, UnsafePointer<Float>, Int32, Int32, Int32, Int32,
                                               UnsafeMutablePointer<Int32>, Int32) -> Int32
    private typealias GreedyFn = @convention(c) (OpaquePointer, UnsafeRawPointer, Int32, Int32, UnsafePointer<Int32>, Int32, Int32,
                                                 Int32, UnsafeMutablePointer<Int32>, UnsafeMutablePointer<Int32>, Int32) -> Int32
    private typealias ErrFn = @convention(c) () -> UnsafePointer<CChar>
    private typealias VocabLoadFn = @convention(c) (UnsafePointer<CChar>, UnsafeMutablePointer<OpaquePointer?>) -> Int32
    private typealias DetokFn = @convention(c) (OpaquePointer, UnsafePointer<Int32>, Int32, Int32, UnsafeMutablePointer<CChar>?,
                                                Int, UnsafeMutablePointer<Int>?) -> Int32

    private func sym<T>(_ name: String) throws -> T {
        guard let p = dlsym(lib, name) else { throw WhisperError(description: "missing symbol \(name)") }
        return unsafeBitCast(p, to: T.self)
    }
    private func message() -> String {
        guard let f: ErrFn = try? sym("wm_last_error") else { return "unknown error" }
        return String(cString: f())
    }
    private func check(_ status: Int32) throws {
        if status != 0 { throw WhisperError(description: "wm status \(status): \(message())") }
    }

    /// was Whisper.swift:17-21 (`decoder(configuration:)`, `encoder(configuration:)`): create the context, load the flat
    /// weight file made by weights.convert_openai_pt (the counterpart of whisper_to_cml.py:6-8,45-52), freeze.
    init(library: String = "libwhisper_mi355x.so", weights: String = "small.wm", dims: wm_dims = .small,
         device: Int32 = 0) throws {
        guard let h = dlopen(library, RTLD_NOW | RTLD_LOCAL) else {
            throw WhisperError(description: "dlopen \(library): \(String(cString: dlerror()))")
        }
        lib = h
        self.dims = dims
        var d = dims
        var c: OpaquePointer?
        let create: CreateFn = unsafeBitCast(dlsym(h, "wm_create")!, to: CreateFn.self)
        let load: LoadFn = unsafeBitCast(dlsym(h, "wm_load_weights")!, to: LoadFn.self)
        let fin: CtxFn = unsafeBitCast(dlsym(h, "wm_finalize")!, to: CtxFn.self)
        let err: ErrFn = unsafeBitCast(dlsym(h, "wm_last_error")!, to: ErrFn.self)
        guard create(&d, device, &c) == 0, let cc = c, load(cc, weights) == 0, fin(cc) == 0 else {
            throw WhisperError(description: String(cString: err()))
        }
        ctx = cc
    }

    /// was Whisper.swift:23-31: spectrogram -> f32 [1, 80, 3000] -> encoder -> [1, 1500, d] (`.var_1385`).
    func encode(audio: [Double]) throws -> [Float] {
        let spec = generateSpectrogram(audio: audio)            // stft.swift:8-19, unchanged (seam #1)
        let mel = spec.map { Float($0) }                        // Whisper.swift:25-28: f64 -> f32 narrowing
        var xa = [Float](repeating: 0, count: 1500 * Int(dims.n_audio_state))
        let f: EncodeFn = try sym("wm_encode")
        try check(f(ctx, mel, 1, &xa, 0 /* WM_MEM_HOST */))
        return xa
    }

    /// was Whisper.swift:33-40: SOT 50258 -> decoder -> first arg-max over ids 50259...50357 -> print the code.
    func decode(audioFeatures: [Float]) throws {
        var idx: Int32 = 0
        let f: LangFn = try sym("wm_detect_language")
        try check(f(ctx, audioFeatures, 1, 50258, 50259, 50357, &idx, 0))
        print(Self.LANGUAGES[Int(idx)])                         // Whisper.swift:39
    }

    /// New surface (BASELINE.json): log-mel -> encoder -> KV-cached greedy decode of `audio` cut into 30 s windows
    /// (the last one zero-padded: ContentView.swift:57-60's rule per window).  Returns the token ids per window.
    func transcribe(audio: [Float], prompt: [Int32] = [50258, 50259, 50359, 50363], maxNew: Int32 = 224,
                    eot: Int32 = 50257) throws -> [[Int32]] {
        let n = 480_000
        let chunks = max(1, (audio.count + n - 1) / n)
        var pcm = [Float](repeating: 0, count: chunks * n)
        pcm.replaceSubrange(0..<audio.count, with: audio)
        var tokens = [Int32](repeating: 0, count: chunks * Int(maxNew))
        var lens = [Int32](repeating: 0, count: chunks)
        let f: GreedyFn = try sym("wm_transcribe_greedy")
        try pcm.withUnsafeBytes { p in
            try check(f(ctx, p.baseAddress!, 1 /* WM_F32 */, Int32(chunks), prompt, Int32(prompt.count), maxNew, eot,
                        &tokens, &lens, 0))
        }
        return (0..<chunks).map { c in Array(tokens[c * Int(maxNew)..<c * Int(maxNew) + Int(lens[c])]) }
    }

    /// The same from a recording on disk -- query.wav as AudioRecorder.swift:56-61 writes it (16 kHz mono 16-bit) -- through the
    /// library's own reader / chunker (wm_wav_*: no AVFoundation on a Linux host), with an optional per-window token budget
    /// (wm_set_token_budgets: a window that has used it up leaves the decode like one that has emitted `eot`).
    func transcribe(wav path: String, prompt: [Int32] = [50258, 50259, 50359, 50363], maxNew: Int32 = 224,
                    eot: Int32 = 50257, budgets: [Int32]? = nil) throws -> [[Int32]] {
        typealias WavOpenFn = @convention(c) (UnsafePointer<CChar>, UnsafeMutablePointer<OpaquePointer?>) -> Int32
        typealias WavCountFn = @convention(c) (OpaquePointer) -> Int32
        typealias WavReadFn = @convention(c) (OpaquePointer, Int32, Int32, UnsafeMutablePointer<Int16>) -> Int32
        typealias BudgetFn = @convention(c) (OpaquePointer, UnsafePointer<Int32>?, Int32) -> Int32
        let open: WavOpenFn = try sym("wm_wav_open")
        let count: WavCountFn = try sym("wm_wav_num_chunks")
        let read: WavReadFn = try sym("wm_wav_read_chunks")
        let close: DestroyFn = try sym("wm_wav_close")
        var w: OpaquePointer?
        try check(open(path, &w))
        defer { close(w!) }
        let chunks = Int(count(w!))
        var pcm = [Int16](repeating: 0, count: chunks * 480_000)
        try check(read(w!, 0, Int32(chunks), &pcm))
        if let b = budgets {
            let setBudgets: BudgetFn = try sym("wm_set_token_budgets")
            try check(setBudgets(ctx, b, Int32(b.count)))          // must be one per window
        }
        var tokens = [Int32](repeating: 0, count: chunks * Int(maxNew))
        var lens = [Int32](repeating: 0, count: chunks)
        let f: GreedyFn = try sym("wm_transcribe_greedy")
        try pcm.withUnsafeBytes { p in
            try check(f(ctx, p.baseAddress!, 0 /* WM_I16 */, Int32(chunks), prompt, Int32(prompt.count), maxNew, eot,
                        &tokens, &lens, 0))
        }
        return (0..<chunks).map { c in Array(tokens[c * Int(maxNew)..<c * Int(maxNew) + Int(lens[c])]) }
    }

    /// Word-level timing inputs (wm_align; openai-whisper find_alignment): for each 30 s window of `audio` and the text
    /// tokens a transcription produced for it (all < eot), the first audio frame (20 ms) of every token plus the end row, and
    /// every token's probability.  Word grouping (split_to_word_tokens, merge_punctuations) is host work: binding.py
    /// word_timestamps.  `alignmentHeads`: a checkpoint's (layer, head) list; nil = the last half of the decoder layers.
    /// Not compiled in this repository (see the top of the file).
    func align(audio: [Float], text: [[Int32]], sotSequence: [Int32] = [50258, 50259, 50359], noTimestamps: Int32 = 50363,
               eot: Int32 = 50257, alignmentHeads: [(Int32, Int32)]? = nil,
               medfiltWidth: Int32 = 7) throws -> (startFrames: [[Int32]], tokenProbs: [[Float]]) {
        typealias HeadsFn = @convention(c) (OpaquePointer, UnsafePointer<Int32>?, UnsafePointer<Int32>?, Int32) -> Int32
        typealias AlignFn = @convention(c) (OpaquePointer, UnsafeRawPointer, Int32, Int32, UnsafePointer<Int32>, Int32, Int32,
                                            Int32, UnsafePointer<Int32>, UnsafePointer<Int32>, Int32, UnsafePointer<Int32>?,
                                            Int32, Float, UnsafeMutablePointer<Int32>, UnsafeMutablePointer<Float>?, Int32) -> Int32
        let n = 480_000
        let chunks = text.count
        var pcm = [Float](repeating: 0, count: chunks * n)
        pcm.replaceSubrange(0..<min(audio.count, chunks * n), with: audio.prefix(chunks * n))
        let maxText = text.map { $0.count }.max() ?? 0
        var flat = [Int32](repeating: 0, count: max(1, chunks * maxText))
        for (c, t) in text.enumerated() { flat.replaceSubrange(c * maxText..<c * maxText + t.count, with: t) }
        let nText = text.map { Int32($0.count) }
        let heads: HeadsFn = try sym("wm_set_alignment_heads")
        let h = alignmentHeads ?? []
        try check(heads(ctx, h.map { $0.0 }, h.map { $0.1 }, Int32(h.count)))
        var start = [Int32](repeating: -1, count: chunks * (maxText + 1))
        var probs = [Float](repeating: 0, count: max(1, chunks * maxText))
        let f: AlignFn = try sym("wm_align")
        try pcm.withUnsafeBytes { p in
            try check(f(ctx, p.baseAddress!, 1 /* WM_F32 */, Int32(chunks), sotSequence, Int32(sotSequence.count),
                        noTimestamps, eot, flat, nText, Int32(maxText), nil, medfiltWidth, 1.0, &start, &probs, 0))
        }
        return ((0..<chunks).map { c in Array(start[c * (maxText + 1)...c * (maxText + 1) + text[c].count]) },
                (0..<chunks).map { c in Array(probs[c * maxText..<c * maxText + text[c].count]) })
    }

    /// The repetition rules of every later transcribe call on this context (wm_set_repetition_rules): `penalty` (> 0; 1 = off)
    /// scales the logit of every id < eot a window has generated in the call, `noRepeatNgramSize` (0 = off, 1 ... 32) bans the
    /// ids < eot that would repeat an n-gram of its generated tokens; the prompt never counts.  The defaults switch them off.
    /// Not compiled in this repository (see the top of the file).
    func setRepetitionRules(penalty: Float = 1.0, noRepeatNgramSize: Int32 = 0, eot: Int32 = 50257) throws {
        typealias RulesFn = @convention(c) (OpaquePointer, Float, Int32, Int32) -> Int32
        let f: RulesFn = try sym("wm_set_repetition_rules")
        try check(f(ctx, penalty, noRepeatNgramSize, eot))
    }

    /// The sampling rules of every later transcribe call on this context that samples (wm_set_sampling_rules; temperature > 0):
    /// `topK` (0 = off) keeps exactly the k best admissible ids, `topP` (1 = off) the shortest prefix of them that holds that share
    /// of their mass, `minP` (0 = off) the ids at least minP times as probable as the best; log-probs stay those of the
    /// untruncated filtered distribution, calls at temperature 0 ignore the rules.  The defaults switch them off.
    /// Not compiled in this repository (see the top of the file).
    func setSamplingRules(topK: Int32 = 0, topP: Float = 1.0, minP: Float = 0.0) throws {
        typealias SamplingFn = @convention(c) (OpaquePointer, Int32, Float, Float) -> Int32
        let f: SamplingFn = try sym("wm_set_sampling_rules")
        try check(f(ctx, topK, topP, minP))
    }

    /// Positions per decoder step (1 ... 8; 1 = the default) of the teacher-forced passes behind align / alignMel / alignWindows /
    /// decodeLogits on this context (wm_set_teacher_panel).  A launch policy: the results are bit-identical for every width.
    /// Not compiled in this repository (see the top of the file).
    func setTeacherPanel(_ width: Int32) throws {
        typealias PanelFn = @convention(c) (OpaquePointer, Int32) -> Int32
        let f: PanelFn = try sym("wm_set_teacher_panel")
        try check(f(ctx, width))
    }

    /// The sequence bias of every later transcribe call on this context (wm_set_sequence_bias): `sequences[i]` carries `bias[i]`
    /// (finite, or -.infinity = a banned sequence), added to the logit of its last token whenever a window's generated tokens end
    /// in its other tokens; `boostPrefixes[i]` biases every proper prefix too, so a phrase is helped from its first token on.
    /// Only ids < eot may end a sequence.  The ids are the caller's tokenizer's: " word" and "word" are different ids, both
    /// variants are the caller's to list.  An empty list switches the bias off.
    /// Not compiled in this repository (see the top of the file).
    func setSequenceBias(sequences: [[Int32]] = [], bias: [Float] = [], boostPrefixes: [Bool] = [], eot: Int32 = 50257) throws {
        typealias BiasFn = @convention(c) (OpaquePointer, UnsafePointer<Int32>?, UnsafePointer<Int32>?, UnsafePointer<Float>?,
                                           UnsafePointer<UInt8>?, Int32, Int32) -> Int32
        let f: BiasFn = try sym("wm_set_sequence_bias")
        precondition(bias.count == sequences.count && (boostPrefixes.isEmpty || boostPrefixes.count == sequences.count))
        if sequences.isEmpty {
            try check(f(ctx, nil, nil, nil, nil, 0, eot))
            return
        }
        var offsets: [Int32] = [0]
        for s in sequences { offsets.append(offsets.last! + Int32(s.count)) }
        let tokens = sequences.flatMap { $0 }
        let flags: [UInt8] = boostPrefixes.map { $0 ? 1 : 0 }
        try check(f(ctx, tokens, offsets, bias, flags.isEmpty ? nil : flags, Int32(sequences.count), eot))
    }

    /// A sequence-bias table PER ROW (wm_set_sequence_bias_tables): `tables[t]` is a list of (sequence, bias, boostPrefixes) as
    /// setSequenceBias takes them, checked and expanded on its own; it replaces the context's single table.  Every later transcribe
    /// call needs setBiasRows in front of it.  An empty list clears the tables.
    /// Not compiled in this repository (see the top of the file).
    func setSequenceBiasTables(_ tables: [[(sequence: [Int32], bias: Float, boostPrefixes: Bool)]], eot: Int32 = 50257) throws {
        typealias TablesFn = @convention(c) (OpaquePointer, UnsafePointer<Int32>?, UnsafePointer<Int32>?, UnsafePointer<Float>?,
                                             UnsafePointer<UInt8>?, UnsafePointer<Int32>?, Int32, Int32) -> Int32
        let f: TablesFn = try sym("wm_set_sequence_bias_tables")
        if tables.isEmpty {
            try check(f(ctx, nil, nil, nil, nil, nil, 0, eot))
            return
        }
        var tableOffsets: [Int32] = [0]
        var offsets: [Int32] = [0]
        var tokens: [Int32] = [], bias: [Float] = [], flags: [UInt8] = []
        for t in tables {
            for e in t {
                tokens += e.sequence
                offsets.append(offsets.last! + Int32(e.sequence.count))
                bias.append(e.bias)
                flags.append(e.boostPrefixes ? 1 : 0)
            }
            tableOffsets.append(Int32(bias.count))
        }
        try check(f(ctx, tokens, offsets, bias, flags, tableOffsets, Int32(tables.count), eot))
    }

    /// The table of every row of the NEXT transcribe call on this context (wm_set_bias_rows; one entry per row of that call,
    /// consumed by it): an index into setSequenceBiasTables' tables, or -1 for a row without a bias.  [] drops a pending map.
    /// Not compiled in this repository (see the top of the file).
    func setBiasRows(_ tableOfRow: [Int32]) throws {
        typealias RowsFn = @convention(c) (OpaquePointer, UnsafePointer<Int32>?, Int32) -> Int32
        let f: RowsFn = try sym("wm_set_bias_rows")
        try check(f(ctx, tableOfRow.isEmpty ? nil : tableOfRow, Int32(tableOfRow.count)))
    }

    /// Temperature and seed of every row of the NEXT transcribe call on this context (wm_set_sampling_rows; one entry per row of
    /// that call, consumed by it): the call's own temperature and seed are then not read; temperature 0 is an arg-max row.
    /// Empty arrays drop a pending map.  Not compiled in this repository (see the top of the file).
    func setSamplingRows(temperatures: [Float], seeds: [UInt64]) throws {
        typealias RowsFn = @convention(c) (OpaquePointer, UnsafePointer<Float>?, UnsafePointer<UInt64>?, Int32) -> Int32
        precondition(temperatures.count == seeds.count)
        let f: RowsFn = try sym("wm_set_sampling_rows")
        try check(f(ctx, temperatures.isEmpty ? nil : temperatures, seeds.isEmpty ? nil : seeds, Int32(temperatures.count)))
    }

    /// Given tokens of the NEXT transcribe call on this context (wm_set_given_tokens; one list per hypothesis row of that call --
    /// B, or B * best_of in the order [B][best_of] --, consumed by it): the row takes them in place of its own choices and
    /// token_logprobs_out holds their log-probs; behind them it decodes freely, an empty list is an ordinary row.  [] drops a
    /// pending table.  Not compiled in this repository (see the top of the file).
    func setGivenTokens(_ rows: [[Int32]]) throws {
        typealias GivenFn = @convention(c) (OpaquePointer, UnsafePointer<Int32>?, Int32, UnsafePointer<Int32>?, Int32) -> Int32
        let f: GivenFn = try sym("wm_set_given_tokens")
        if rows.isEmpty {
            try check(f(ctx, nil, 0, nil, 0))
            return
        }
        let stride = max(1, rows.map { $0.count }.max()!)
        var tokens = [Int32](repeating: 0, count: rows.count * stride)
        for (r, row) in rows.enumerated() {
            for (i, t) in row.enumerated() { tokens[r * stride + i] = t }
        }
        try check(f(ctx, tokens, Int32(stride), rows.map { Int32($0.count) }, Int32(rows.count)))
    }

    /// Generated positions per decoder step over the given tokens of a transcribe call (wm_set_given_panel; 1 ... 8, 1 = the
    /// default).  A launch policy of the context, not consumed by calls: every output has the bits of width 1, and no call
    /// fails because of it.  Not compiled in this repository (see the top of the file).
    func setGivenPanel(_ width: Int32) throws {
        typealias PanelFn = @convention(c) (OpaquePointer, Int32) -> Int32
        let f: PanelFn = try sym("wm_set_given_panel")
        try check(f(ctx, width))
    }

    /// openai-whisper's whole-recording log-mel (wm_logmel_long; log_mel_spectrogram(audio, padding=480000)) of each
    /// recording, f32, host memory: recording r -> [nMels][(count + 480000) / 160] row-major.
    /// Not compiled in this repository (see the top of the file).
    func logMelLong(recordings: [[Float]], nMels: Int32 = 80) throws -> [[Float]] {
        typealias LongFn = @convention(c) (OpaquePointer, UnsafeRawPointer?, Int32, UnsafePointer<Int64>, Int32, Int32,
                                           UnsafeMutablePointer<Float>, Int32) -> Int32
        var offsets: [Int64] = [0]
        for r in recordings { offsets.append(offsets.last! + Int64(r.count)) }
        let frames = recordings.map { ($0.count + 480_000) / 160 }
        let pcm = recordings.flatMap { $0 }
        var out = [Float](repeating: 0, count: max(1, frames.reduce(0, +) * Int(nMels)))
        let f: LongFn = try sym("wm_logmel_long")
        try pcm.withUnsafeBytes { p in
            try check(f(ctx, p.baseAddress, 1 /* WM_F32 */, offsets, Int32(recordings.count), nMels, &out, 0))
        }
        var result: [[Float]] = []
        var at = 0
        for t in frames {
            result.append(Array(out[at..<at + t * Int(nMels)]))
            at += t * Int(nMels)
        }
        return result
    }

    // ---- live streams (wm_streams_*): appended samples become log-mel frames incrementally on the device ----
    typealias StreamsCreateFn = @convention(c) (OpaquePointer, Int32, Int32, Int32, UnsafeMutablePointer<OpaquePointer?>) -> Int32
    typealias StreamsFreeFn = @convention(c) (OpaquePointer, OpaquePointer?) -> Int32
    typealias StreamsPushFn = @convention(c) (OpaquePointer, OpaquePointer, UnsafeRawPointer?, Int32, UnsafePointer<Int64>,
                                              Int32) -> Int32
    typealias StreamsResetFn = @convention(c) (OpaquePointer, OpaquePointer, Int32) -> Int32
    typealias StreamsFramesFn = @convention(c) (OpaquePointer, UnsafeMutablePointer<Int64>?, UnsafeMutablePointer<Int64>?,
                                                UnsafeMutablePointer<Int64>?, UnsafeMutablePointer<Int64>?) -> Int32
    typealias StreamsWindowFn = @convention(c) (OpaquePointer, OpaquePointer, Int32, UnsafePointer<Int32>, UnsafePointer<Int64>,
                                                UnsafePointer<Int32>, UnsafeMutablePointer<Float>, UnsafePointer<Int64>,
                                                Int32) -> Int32

    /// A set of `count` live streams (wm_streams_create); free it with streamsFree before the context goes.
    /// Not compiled in this repository (see the top of the file).
    func streamsCreate(count: Int32, nMels: Int32 = 80, capacityFrames: Int32 = 3003) throws -> OpaquePointer {
        var set: OpaquePointer?
        let f: StreamsCreateFn = try sym("wm_streams_create")
        try check(f(ctx, count, nMels, capacityFrames, &set))
        return set!
    }

    func streamsFree(_ set: OpaquePointer) throws {
        let f: StreamsFreeFn = try sym("wm_streams_free")
        try check(f(ctx, set))
    }

    /// Appends pieces[s] (f32, 16 kHz; empty: nothing) to stream s: one launch for all streams (wm_streams_push).
    func streamsPush(_ set: OpaquePointer, pieces: [[Float]]) throws {
        var offsets: [Int64] = [0]
        for p in pieces { offsets.append(offsets.last! + Int64(p.count)) }
        let pcm = pieces.flatMap { $0 }
        let f: StreamsPushFn = try sym("wm_streams_push")
        try pcm.withUnsafeBytes { p in
            try check(f(ctx, set, p.baseAddress, 1 /* WM_F32 */, offsets, 0))
        }
    }

    func streamsReset(_ set: OpaquePointer, stream: Int32) throws {
        let f: StreamsResetFn = try sym("wm_streams_reset")
        try check(f(ctx, set, stream))
    }

    /// (samples, final frames, available frames, first kept frame) of each of the set's `count` streams (wm_streams_frames).
    func streamsFrames(_ set: OpaquePointer, count: Int) throws -> (samples: [Int64], final: [Int64], avail: [Int64], firstKept: [Int64]) {
        var n = [Int64](repeating: 0, count: count), fin = n, av = n, k = n
        let f: StreamsFramesFn = try sym("wm_streams_frames")
        try check(f(set, &n, &fin, &av, &k))
        return (n, fin, av, k)
    }

    /// Frames [first, first + frames) of a stream, normalised as a recording that is the window (wm_streams_window), host
    /// memory: [nMels][frames] row-major -- what the mel entries take with seek 0.
    func streamsWindow(_ set: OpaquePointer, stream: Int32, first: Int64, frames: Int32, nMels: Int32 = 80) throws -> [Float] {
        var out = [Float](repeating: 0, count: Int(nMels) * Int(frames))
        let f: StreamsWindowFn = try sym("wm_streams_window")
        try check(f(ctx, set, 1, [stream], [first], [frames], &out, [0], 0))
        return out
    }

    /// Recordings at their own sample rate and channel count -> 16 kHz mono f32 (wm_resample_16k: one launch, the polyphase
    /// Kaiser-sinc resampler of DESIGN.md section 12), host memory.  recordings[r] holds interleaved frames of channels[r]
    /// channels at sampleRates[r] Hz; the result feeds logMelLong as it is.
    /// Not compiled in this repository (see the top of the file).
    func resample16k(recordings: [[Float]], channels: [Int32], sampleRates: [Int32]) throws -> [[Float]] {
        typealias ResampleFn = @convention(c) (OpaquePointer, UnsafeRawPointer?, Int32, UnsafePointer<Int64>, UnsafePointer<Int32>,
                                               UnsafePointer<Int32>, Int32, UnsafeMutablePointer<Float>, Int32) -> Int32
        typealias OutLenFn = @convention(c) (Int64, Int32) -> Int64
        let outLen: OutLenFn = try sym("wm_resample_out_len")
        var offsets: [Int64] = [0]
        for r in recordings { offsets.append(offsets.last! + Int64(r.count)) }
        let lens = try recordings.indices.map { r -> Int in
            let n = outLen(Int64(recordings[r].count) / Int64(max(channels[r], 1)), sampleRates[r])
            if n < 0 { throw WhisperError(description: "unsupported sample rate \(sampleRates[r])") }
            return Int(n)
        }
        let pcm = recordings.flatMap { $0 }
        var out = [Float](repeating: 0, count: max(1, lens.reduce(0, +)))
        let f: ResampleFn = try sym("wm_resample_16k")
        try pcm.withUnsafeBytes { p in
            try check(f(ctx, p.baseAddress, 1 /* WM_F32 */, offsets, channels, sampleRates, Int32(recordings.count), &out, 0))
        }
        var result: [[Float]] = []
        var at = 0
        for n in lens {
            result.append(Array(out[at..<at + n]))
            at += n
        }
        return result
    }

    /// resample16k with a channel matrix (wm_resample_16k_mix, DESIGN.md section 24), host memory.  rows[r] is the number of
    /// output signals of recording r and mix holds their weight rows back to back -- channels[r] weights each, in
    /// (recording, row) order; the identity gives one signal per channel.  Returns the signals in (recording, row) order.
    /// Not compiled in this repository (see the top of the file).
    func resample16kMix(recordings: [[Float]], channels: [Int32], sampleRates: [Int32], rows: [Int32], mix: [Float]) throws -> [[Float]] {
        typealias MixFn = @convention(c) (OpaquePointer, UnsafeRawPointer?, Int32, UnsafePointer<Int64>, UnsafePointer<Int32>,
                                          UnsafePointer<Int32>, Int32, UnsafePointer<Int32>, UnsafePointer<Float>,
                                          UnsafeMutablePointer<Float>, Int32) -> Int32
        typealias OutLenFn = @convention(c) (Int64, Int32) -> Int64
        let outLen: OutLenFn = try sym("wm_resample_out_len")
        var offsets: [Int64] = [0]
        for r in recordings { offsets.append(offsets.last! + Int64(r.count)) }
        var lens: [Int] = []
        for r in recordings.indices {
            let n = outLen(Int64(recordings[r].count) / Int64(max(channels[r], 1)), sampleRates[r])
            if n < 0 { throw WhisperError(description: "unsupported sample rate \(sampleRates[r])") }
            lens += [Int](repeating: Int(n), count: Int(rows[r]))
        }
        let pcm = recordings.flatMap { $0 }
        var out = [Float](repeating: 0, count: max(1, lens.reduce(0, +)))
        let f: MixFn = try sym("wm_resample_16k_mix")
        try pcm.withUnsafeBytes { p in
            try check(f(ctx, p.baseAddress, 1 /* WM_F32 */, offsets, channels, sampleRates, Int32(recordings.count), rows, mix, &out, 0))
        }
        var result: [[Float]] = []
        var at = 0
        for n in lens {
            result.append(Array(out[at..<at + n]))
            at += n
        }
        return result
    }

    /// Per-channel activity (wm_channel_activity): per 16 kHz signal, the sum of |y| over every 160 samples -- one value per
    /// mel frame --, host memory.  Returns one track of ceil(count / 160) values per signal.
    /// Not compiled in this repository (see the top of the file).
    func channelActivity(signals: [[Float]]) throws -> [[Float]] {
        typealias ActivityFn = @convention(c) (OpaquePointer, UnsafePointer<Float>, UnsafePointer<Int64>, Int32,
                                               UnsafeMutablePointer<Float>, Int32) -> Int32
        var offsets: [Int64] = [0]
        for s in signals { offsets.append(offsets.last! + Int64(s.count)) }
        let lens = signals.map { ($0.count + 159) / 160 }
        let pcm = signals.flatMap { $0 } + [0]   // (never empty: a base address to pass)
        var out = [Float](repeating: 0, count: max(1, lens.reduce(0, +)))
        let f: ActivityFn = try sym("wm_channel_activity")
        try check(f(ctx, pcm, offsets, Int32(signals.count), &out, 0))
        var result: [[Float]] = []
        var at = 0
        for n in lens {
            result.append(Array(out[at..<at + n]))
            at += n
        }
        return result
    }

    /// wm_vad_params (include/whisper_mi355x.h), field for field; `VadParams.defaults()` is wm_vad_default_params.  The
    /// defaults are not validated on real speech.
    struct VadParams {
        var qFloor: Float = 0, qPeak: Float = 0, minRange: Float = 0, onFrac: Float = 0, offFrac: Float = 0
        var minSpeech: Int32 = 0, minSilence: Int32 = 0, speechPad: Int32 = 0
    }

    /// wm_vad_default_params.  Not compiled in this repository (see the top of the file).
    func vadDefaultParams() throws -> VadParams {
        typealias DefaultsFn = @convention(c) (UnsafeMutableRawPointer?) -> Void
        let f: DefaultsFn = try sym("wm_vad_default_params")
        var p = VadParams()
        withUnsafeMutableBytes(of: &p) { f($0.baseAddress) }
        return p
    }

    /// Smoothed band energy per frame of logMelLong's output (wm_vad_energy: one launch for all recordings), host memory.
    /// mel: the recordings' [nMels][frames[r]] blocks back to back; nFrames[r]: the frames to do (the content frames,
    /// frames[r] - 3000); band: the mel rows [lo, hi); smooth: odd, 1 ... 31.  Returns one track per recording.
    /// Not compiled in this repository (see the top of the file).
    func vadEnergy(mel: [Float], frames: [Int32], nFrames: [Int32], nMels: Int32, bandLo: Int32, bandHi: Int32,
                   smooth: Int32 = 5) throws -> [[Float]] {
        typealias VadFn = @convention(c) (OpaquePointer, UnsafePointer<Float>, UnsafePointer<Int64>, UnsafePointer<Int32>,
                                          UnsafePointer<Int32>, Int32, Int32, Int32, Int32, Int32, UnsafeMutablePointer<Float>?,
                                          UnsafeMutablePointer<Float>, Int32) -> Int32
        var base: [Int64] = []
        var at: Int64 = 0
        for t in frames { base.append(at); at += Int64(t) * Int64(nMels) }
        var out = [Float](repeating: 0, count: max(1, nFrames.reduce(0) { $0 + Int($1) }))
        let f: VadFn = try sym("wm_vad_energy")
        try check(f(ctx, mel, base, frames, nFrames, Int32(frames.count), nMels, bandLo, bandHi, smooth, nil, &out, 0))
        var result: [[Float]] = []
        var o = 0
        for n in nFrames {
            result.append(Array(out[o..<o + Int(n)]))
            o += Int(n)
        }
        return result
    }

    /// Speech spans [start, end) in frames of one recording's energy track (wm_vad_segments: host only): a sizing call,
    /// then the call that fills.  Not compiled in this repository (see the top of the file).
    func vadSegments(track: [Float], params: VadParams) throws -> [(start: Int32, end: Int32)] {
        typealias SegFn = @convention(c) (UnsafePointer<Float>?, Int64, UnsafeRawPointer?, UnsafeMutablePointer<Int32>?, Int32,
                                          UnsafeMutablePointer<Int32>, UnsafeMutablePointer<Float>?) -> Int32
        let f: SegFn = try sym("wm_vad_segments")
        var p = params
        var n: Int32 = 0
        try withUnsafeBytes(of: &p) { try check(f(track, Int64(track.count), $0.baseAddress, nil, 0, &n, nil)) }
        var pairs = [Int32](repeating: 0, count: max(2, 2 * Int(n)))
        try withUnsafeBytes(of: &p) { try check(f(track, Int64(track.count), $0.baseAddress, &pairs, n, &n, nil)) }
        return (0..<Int(n)).map { (pairs[2 * $0], pairs[2 * $0 + 1]) }
    }

    /// A RIFF/WAVE file of any rate, 1 ... 8 channels, integer PCM 8 / 16 / 24 / 32 bits or IEEE float 32 / 64 bits
    /// (wm_audio_*: the general reader beside wm_wav_*): interleaved f32 frames, the rate and the channel count --
    /// the arguments of resample16k.  Not compiled in this repository (see the top of the file).
    func readAudio(path: String) throws -> (samples: [Float], sampleRate: Int32, channels: Int32) {
        typealias AudioOpenFn = @convention(c) (UnsafePointer<CChar>, UnsafeMutablePointer<OpaquePointer?>) -> Int32
        typealias AudioIntFn = @convention(c) (OpaquePointer?) -> Int32
        typealias AudioFramesFn = @convention(c) (OpaquePointer?) -> Int64
        typealias AudioReadFn = @convention(c) (OpaquePointer?, Int64, Int64, UnsafeMutablePointer<Float>) -> Int32
        typealias AudioCloseFn = @convention(c) (OpaquePointer?) -> Void
        let open: AudioOpenFn = try sym("wm_audio_open")
        let rate: AudioIntFn = try sym("wm_audio_sample_rate")
        let chans: AudioIntFn = try sym("wm_audio_channels")
        let frames: AudioFramesFn = try sym("wm_audio_num_frames")
        let read: AudioReadFn = try sym("wm_audio_read")
        let close: AudioCloseFn = try sym("wm_audio_close")
        var audio: OpaquePointer?
        try check(open(path, &audio))
        defer { close(audio) }
        let n = frames(audio), c = chans(audio)
        var out = [Float](repeating: 0, count: max(1, Int(n) * Int(c)))
        try check(read(audio, 0, n, &out))
        return (Array(out[0..<Int(n) * Int(c)]), rate(audio), c)
    }

    /// One decode step of the long-form loop (wm_transcribe_mel): row b decodes mel[:, seek[b] ..< seek[b] + nFrames[b]] of
    /// the recording block at element melBase[b] (melLen[b] frames) with its own prompt; temperature 0, host memory.
    /// Returns each row's generated tokens.  Not compiled in this repository (see the top of the file).
    func transcribeMel(mel: [Float], melBase: [Int64], melLen: [Int32], seek: [Int32], nFrames: [Int32],
                       prompts: [[Int32]], maxNew: Int32, eot: Int32) throws -> [[Int32]] {
        typealias MelFn = @convention(c) (OpaquePointer, UnsafePointer<Float>, UnsafePointer<Int64>, UnsafePointer<Int32>,
                                          UnsafePointer<Int32>, UnsafePointer<Int32>, Int32, UnsafePointer<Int32>, Int32,
                                          UnsafePointer<UInt32>?, Int32, Int32, UnsafeRawPointer?,
                                          UnsafeMutablePointer<Int32>, UnsafeMutablePointer<Int32>,
                                          UnsafeMutablePointer<Float>?, UnsafeMutablePointer<Float>?, Int32) -> Int32
        let rows = melBase.count
        let nPrompt = prompts.first?.count ?? 0
        let flat = prompts.flatMap { $0 }
        var tokens = [Int32](repeating: 0, count: rows * Int(maxNew))
        var lens = [Int32](repeating: 0, count: rows)
        let f: MelFn = try sym("wm_transcribe_mel")
        try check(f(ctx, mel, melBase, melLen, seek, nFrames, Int32(rows), flat, Int32(nPrompt), nil, maxNew, eot, nil,
                    &tokens, &lens, nil, nil, 0))
        return (0..<rows).map { r in Array(tokens[r * Int(maxNew)..<r * Int(maxNew) + Int(lens[r])]) }
    }

    /// The same step with prompts of different lengths (wm_transcribe_mel_ragged): what condition_on_previous_text needs,
    /// every row's prompt being [sot_prev, *its recording's previous text, sot, language, task] (sotTail 3) or
    /// [sot, language, task].  Returns each row's generated tokens.  Not compiled in this repository.
    func transcribeMelRagged(mel: [Float], melBase: [Int64], melLen: [Int32], seek: [Int32], nFrames: [Int32],
                             prompts: [[Int32]], sotTail: Int32, maxNew: Int32, eot: Int32) throws -> [[Int32]] {
        typealias RaggedFn = @convention(c) (OpaquePointer, UnsafePointer<Float>, UnsafePointer<Int64>, UnsafePointer<Int32>,
                                             UnsafePointer<Int32>, UnsafePointer<Int32>, Int32, UnsafePointer<Int32>, Int32,
                                             UnsafePointer<Int32>, Int32, UnsafePointer<UInt32>?, Int32, Int32,
                                             UnsafeRawPointer?, UnsafeMutablePointer<Int32>, UnsafeMutablePointer<Int32>,
                                             UnsafeMutablePointer<Float>?, UnsafeMutablePointer<Float>?, Int32) -> Int32
        let rows = melBase.count
        let stride = prompts.map { $0.count }.max() ?? 0
        let lens = prompts.map { Int32($0.count) }
        let flat = prompts.flatMap { $0 + [Int32](repeating: 0, count: stride - $0.count) }
        var tokens = [Int32](repeating: 0, count: rows * Int(maxNew))
        var outLens = [Int32](repeating: 0, count: rows)
        let f: RaggedFn = try sym("wm_transcribe_mel_ragged")
        try check(f(ctx, mel, melBase, melLen, seek, nFrames, Int32(rows), flat, Int32(stride), lens, sotTail, nil, maxNew,
                    eot, nil, &tokens, &outLens, nil, nil, 0))
        return (0..<rows).map { r in Array(tokens[r * Int(maxNew)..<r * Int(maxNew) + Int(outLens[r])]) }
    }

    /// openai-whisper's best_of on the same step (wm_transcribe_mel_best_of): bestOf sampled candidates per window that share
    /// the window's encoder pass and cross-attention cache, ranked by the library (lengthPenalty nil = openai-whisper's None).
    /// Uniform prompts of one length (sotTail nil) or ragged ones.  Returns, per window, the generated tokens of every
    /// candidate and the index of the best one.  Not compiled in this repository.
    func transcribeMelBestOf(mel: [Float], melBase: [Int64], melLen: [Int32], seek: [Int32], nFrames: [Int32],
                             prompts: [[Int32]], sotTail: Int32?, bestOf: Int32, lengthPenalty: Float?, temperature: Float,
                             seed: UInt64, maxNew: Int32, eot: Int32) throws -> (candidates: [[[Int32]]], best: [Int32]) {
        typealias BestOfFn = @convention(c) (OpaquePointer, UnsafePointer<Float>, UnsafePointer<Int64>, UnsafePointer<Int32>,
                                             UnsafePointer<Int32>, UnsafePointer<Int32>, Int32, UnsafePointer<Int32>, Int32,
                                             UnsafePointer<Int32>?, Int32, UnsafePointer<UInt32>?, Int32, Float, Int32, Int32,
                                             UnsafeRawPointer?, UnsafeMutablePointer<Int32>, UnsafeMutablePointer<Int32>,
                                             UnsafeMutablePointer<Float>?, UnsafeMutablePointer<Float>?,
                                             UnsafeMutablePointer<Int32>?, Int32) -> Int32
        struct DecodeOpts { var temperature: Float; var seed: UInt64; var noSpeechToken: Int32; var sotIndex: Int32 }   // wm_decode_opts
        let rows = melBase.count, n = Int(bestOf), m = Int(maxNew)
        let stride = prompts.map { $0.count }.max() ?? 0
        let lens = prompts.map { Int32($0.count) }
        let flat = prompts.flatMap { $0 + [Int32](repeating: 0, count: stride - $0.count) }
        var opts = DecodeOpts(temperature: temperature, seed: seed, noSpeechToken: -1, sotIndex: 0)
        var tokens = [Int32](repeating: 0, count: rows * n * m)
        var outLens = [Int32](repeating: 0, count: rows * n)
        var best = [Int32](repeating: 0, count: rows)
        let f: BestOfFn = try sym("wm_transcribe_mel_best_of")
        let st = withUnsafePointer(to: &opts) { o in
            f(ctx, mel, melBase, melLen, seek, nFrames, Int32(rows), flat, Int32(stride), sotTail == nil ? nil : lens,
              sotTail ?? 0, nil, bestOf, lengthPenalty ?? Float.nan, maxNew, eot, UnsafeRawPointer(o), &tokens, &outLens, nil, nil,
              &best, 0)
        }
        try check(st)
        let cands = (0..<rows).map { r in (0..<n).map { s in Array(tokens[(r * n + s) * m..<(r * n + s) * m + Int(outLens[r * n + s])]) } }
        return (cands, best)
    }

    /// openai-whisper's beam search on the same step (wm_transcribe_mel_beam): beamSize beams per window that share the
    /// window's encoder pass and cross-attention cache; patience nil = 1.0 (maxCandidates = round(beamSize * patience)),
    /// lengthPenalty nil = openai-whisper's None.  Uniform prompts of one length (sotTail nil) or ragged ones.  Returns, per
    /// window, the tokens and the summed log-prob of every hypothesis and the index of the best one.  Not compiled in this
    /// repository.
    func transcribeMelBeam(mel: [Float], melBase: [Int64], melLen: [Int32], seek: [Int32], nFrames: [Int32], prompts: [[Int32]],
                           sotTail: Int32?, beamSize: Int32, patience: Float?, lengthPenalty: Float?, maxNew: Int32,
                           eot: Int32) throws -> (hypotheses: [[[Int32]]], sums: [[Float]], best: [Int32]) {
        typealias BeamFn = @convention(c) (OpaquePointer, UnsafePointer<Float>, UnsafePointer<Int64>, UnsafePointer<Int32>,
                                           UnsafePointer<Int32>, UnsafePointer<Int32>, Int32, UnsafePointer<Int32>, Int32,
                                           UnsafePointer<Int32>?, Int32, Int32, Int32, Float, Int32, Int32, UnsafeRawPointer?,
                                           UnsafeMutablePointer<Int32>, UnsafeMutablePointer<Int32>, UnsafeMutablePointer<Int32>,
                                           UnsafeMutablePointer<Float>, UnsafeMutablePointer<Float>?, UnsafeMutablePointer<Float>?,
                                           UnsafeMutablePointer<Int32>?, Int32) -> Int32
        let maxCand = Int32((Float(beamSize) * (patience ?? 1.0)).rounded(.toNearestOrEven))   // Python's round
        let rows = melBase.count, s = Int(max(beamSize, maxCand)), m = Int(maxNew)
        let stride = prompts.map { $0.count }.max() ?? 0
        let lens = prompts.map { Int32($0.count) }
        let flat = prompts.flatMap { $0 + [Int32](repeating: 0, count: stride - $0.count) }
        var tokens = [Int32](repeating: 0, count: rows * s * m)
        var outLens = [Int32](repeating: 0, count: rows * s)
        var nHyp = [Int32](repeating: 0, count: rows)
        var sums = [Float](repeating: 0, count: rows * s)
        var best = [Int32](repeating: 0, count: rows)
        let f: BeamFn = try sym("wm_transcribe_mel_beam")
        try check(f(ctx, mel, melBase, melLen, seek, nFrames, Int32(rows), flat, Int32(stride), sotTail == nil ? nil : lens,
                    sotTail ?? 0, beamSize, maxCand, lengthPenalty ?? Float.nan, maxNew, eot, nil, &tokens, &outLens, &nHyp, &sums,
                    nil, nil, &best, 0))
        let hyps = (0..<rows).map { r in (0..<Int(nHyp[r])).map { h in Array(tokens[(r * s + h) * m..<(r * s + h) * m + Int(outLens[r * s + h])]) } }
        return (hyps, (0..<rows).map { r in Array(sums[r * s..<r * s + Int(nHyp[r])]) }, best)
    }

    /// Word-level timing inputs of the windows of a long-form round (wm_align_mel): the window description of
    /// transcribeMel, one start sequence per row ([sot, language, task] with the row's own language) and the text tokens the
    /// round decoded for each window (all < eot).  Same outputs as align.  The word rules (add_word_timestamps) and the
    /// word-driven seek are host work: binding.py window_word_timestamps / transcribe_long.  Not compiled in this repository.
    func alignMel(mel: [Float], melBase: [Int64], melLen: [Int32], seek: [Int32], nFrames: [Int32],
                  sotSequences: [[Int32]], text: [[Int32]], noTimestamps: Int32 = 50363, eot: Int32 = 50257,
                  medfiltWidth: Int32 = 7) throws -> (startFrames: [[Int32]], tokenProbs: [[Float]]) {
        typealias AlignMelFn = @convention(c) (OpaquePointer, UnsafePointer<Float>, UnsafePointer<Int64>, UnsafePointer<Int32>,
                                               UnsafePointer<Int32>, UnsafePointer<Int32>, Int32, UnsafePointer<Int32>, Int32,
                                               Int32, Int32, UnsafePointer<Int32>, UnsafePointer<Int32>, Int32, Int32, Float,
                                               UnsafeMutablePointer<Int32>, UnsafeMutablePointer<Float>?, Int32) -> Int32
        let rows = melBase.count
        let nSot = sotSequences.first?.count ?? 0
        let sot = sotSequences.flatMap { $0 }
        let maxText = text.map { $0.count }.max() ?? 0
        var flat = [Int32](repeating: 0, count: max(1, rows * maxText))
        for (r, t) in text.enumerated() { flat.replaceSubrange(r * maxText..<r * maxText + t.count, with: t) }
        let nText = text.map { Int32($0.count) }
        var start = [Int32](repeating: -1, count: rows * (maxText + 1))
        var probs = [Float](repeating: 0, count: max(1, rows * maxText))
        let f: AlignMelFn = try sym("wm_align_mel")
        try check(f(ctx, mel, melBase, melLen, seek, nFrames, Int32(rows), sot, Int32(nSot), noTimestamps, eot, flat, nText,
                    Int32(maxText), medfiltWidth, 1.0, &start, &probs, 0))
        return ((0..<rows).map { r in Array(start[r * (maxText + 1)...r * (maxText + 1) + text[r].count]) },
                (0..<rows).map { r in Array(probs[r * maxText..<r * maxText + text[r].count]) })
    }

    /// ids -> text with the tokenizer's vocab.json (wm_vocab_load / wm_detokenize; no vocabulary ships with the library).
    func text(of ids: [Int32], vocabJSON: String) throws -> String {
        let load: VocabLoadFn = try sym("wm_vocab_load")
        let detok: DetokFn = try sym("wm_detokenize")
        let free: DestroyFn = try sym("wm_vocab_free")
        var v: OpaquePointer?
        try check(load(vocabJSON, &v))
        defer { free(v!) }
        var need = 0
        try check(detok(v!, ids, Int32(ids.count), 1, nil, 0, &need))
        var buf = [CChar](repeating: 0, count: need)
        try check(detok(v!, ids, Int32(ids.count), 1, &buf, need, nil))
        return String(cString: buf)
    }
}

// ContentView.swift:61-62 (`whisper.encode(audio:)`, `whisper.decode(audioFeatures:)`) compiles unchanged against this
// struct, except that the intermediate is `[Float]` instead of `MLMultiArray`.
